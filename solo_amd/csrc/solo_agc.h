// solo_agc.h -- per-row level control and peak limiter for decoded rows (solo_agc, include/solo_mi355x.h).
//
// The stage between solo_vad and the selection / the mix: it reads the compact rows int16 [n][P][L] that solo_playout_tick writes, the
// levels and activities that solo_vad wrote for them, and writes rows of the same layout whose speech sits at target_level -dBov and
// whose samples never exceed `ceiling`.  Integer arithmetic with a total rule (include/solo_mi355x.h states it; tests/agc_model.py is
// the same rule in plain Python integers): the output is a pure function of inputs and state.
//
// The state record of a row is 16 words: run, spl_q8 (smoothed speech level, -dBov Q8), gain_q8 (dB Q8), g_q16 (the linear gain at the
// last sample of the previous packet), env_q15 (the limiter envelope at the end of the previous packet), eleven words that the
// stage never writes.  gain_q8, g_q16 and env_q15 are clamped when they are read, so no record can index outside a table.
//
// The kernel: ONE wavefront per row, the row's packets in sequence, lane b = block b of 32 samples (L / 32 <= 60 blocks).  A lane
// loads its 64 bytes as four 16-byte loads and keeps them in registers from the load to the store; its block's peak is local; the
// limiter's recursion e_b = min(a'_b, e_{b-1} + rel) is evaluated in its closed form
//
//     e_b = b rel + min(e_{-1} + rel, min_{j <= b}(a'_j - j rel))
//
// with ONE prefix minimum over the lanes (sx_agc_prefix_min: four DPP row shifts and the two row broadcasts, the steps of wv_scan_incl
// with min in the place of +), e_{b-1} comes from the neighbouring lane, and the energies go through wv_sum64.  What crosses lanes is
// written as a function of a per-lane array of SX_AGC_PL values (1 on the device; all 60 blocks in the 1-lane host build, where the
// same functions are plain loops), so that the host build runs the same text (tests/agc_host.cpp).
#pragma once
#include <stddef.h>
#include "solo_vad.h"           // sx_vad_level
#include "solo_agc_tables.inc"

#define SX_AGC_STATE_WORDS 16
#define SX_AGC_MIN_PACKET 256
#define SX_AGC_MAX_PACKET 1920
#define SX_AGC_MAX_BLOCKS (SX_AGC_MAX_PACKET / 32)
#define SX_AGC_PL ((SX_AGC_MAX_BLOCKS + SX_NLANES - 1) / SX_NLANES)     // blocks a lane holds
#define SX_AGC_MAX_GAIN_Q8 7680                                         // 30 dB
#define SX_AGC_ONE_Q15 32768

typedef solo_agc_params_t SxAgcParams;
typedef solo_agc_count_t SxAgcCount;
static_assert(sizeof(SxAgcParams) == 40 && sizeof(SxAgcCount) == 16, "solo_agc_params_t, solo_agc_count_t layout");

// word w of the record the create and reset calls leave
SX_HD i32 sx_agc_init_word(int w) { return w == 3 ? 65536 : (w == 4 ? SX_AGC_ONE_Q15 : 0); }

static inline bool sx_agc_params_ok(const SxAgcParams* p) {
    return p && p->target_level >= 0 && p->target_level <= 127 && p->max_boost_db >= 0 && p->max_boost_db <= 30 && p->max_cut_db >= 0 && p->max_cut_db <= 30 &&
           p->sa_on_q8 >= 0 && p->sa_on_q8 <= 255 && p->gate_level >= 0 && p->gate_level <= 127 && p->alpha_q8 >= 1 && p->alpha_q8 <= 256 &&
           p->slew_up_q8 >= 0 && p->slew_up_q8 <= SX_AGC_MAX_GAIN_Q8 && p->slew_down_q8 >= 0 && p->slew_down_q8 <= SX_AGC_MAX_GAIN_Q8 &&
           p->ceiling >= 1 && p->ceiling <= 32767 && p->release_q15 >= 0 && p->release_q15 <= SX_AGC_ONE_Q15;
}
static inline bool sx_agc_packet_ok(i32 L) { return L >= SX_AGC_MIN_PACKET && L <= SX_AGC_MAX_PACKET && L % 32 == 0; }
// what the host checks of a solo_agc call before it enqueues anything (rows / count: the call's d_rows and d_count)
static inline bool sx_agc_call_ok(i32 n_rows, const void* rows, i32 n, const void* pcm_in, i32 n_packets, i32 packet_samples, const void* sa, i32 frames,
                                  const SxAgcParams* p, const void* pcm_out, const void* count) {
    if (!pcm_in || !pcm_out || !sx_agc_params_ok(p) || (rows && !count) || n <= 0 || n > n_rows || n_packets <= 0) return false;
    if (!sx_agc_packet_ok(packet_samples) || (sa && frames <= 0)) return false;
    const i64 np = (i64)n * (i64)n_packets;
    if (np * packet_samples >= ((i64)1 << 31) || (sa && np * frames >= ((i64)1 << 31))) return false;
    if (((uintptr_t)pcm_in | (uintptr_t)pcm_out) & 15) return false;
    const uintptr_t a = (uintptr_t)pcm_in, b = (uintptr_t)pcm_out, bytes = (uintptr_t)(np * packet_samples * 2);
    return a == b || a + bytes <= b || b + bytes <= a;      // in place, or apart
}

// a gain of d / 256 dB, d in [-7680, 7680], as a Q16 factor
SX_HD i32 sx_agc_lin(i32 d) {
    const i32 u = d + SX_AGC_MAX_GAIN_Q8;
    return (i32)(((i64)T_agc_db[u >> 8] * (i64)T_agc_frac[u & 255] + 32768) >> 16);
}
SX_HD i32 sx_agc_clamp(i32 v, i32 lo, i32 hi) { return sx_min(sx_max(v, lo), hi); }
SX_HD i64 sx_agc_clamp64(i64 v, i64 lo, i64 hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- what crosses lanes: block b's value is v[b / SX_NLANES] of lane b % SX_NLANES ------------------------------------------------------
// Inclusive prefix minimum over the 64 lanes.  The host form of the six steps on an array of 64 values (what tests/test_agc_model.py
// checks against a running minimum): a lane whose source lies outside its 16-lane row, or whose row a broadcast does not reach, keeps
// its value.
SX_HD void sx_agc_prefix_min_steps(i32 v[64]) {
    for (int sh = 1; sh < 16; sh <<= 1) {                   // row_shr:sh, reading the values of before the step
        i32 t[64];
        for (int l = 0; l < 64; l++) t[l] = (l & 15) >= sh ? v[l - sh] : v[l];
        for (int l = 0; l < 64; l++) v[l] = sx_min(v[l], t[l]);
    }
    const i32 b15[2] = {v[15], v[47]};                      // row_bcast:15 row_mask:0xa
    for (int l = 0; l < 64; l++) if ((l >> 4) & 1) v[l] = sx_min(v[l], b15[l >> 5]);
    const i32 b31 = v[31];                                  // row_bcast:31 row_mask:0xc
    for (int l = 32; l < 64; l++) v[l] = sx_min(v[l], b31);
}
#if defined(__HIP_DEVICE_COMPILE__) && SX_NLANES == 64
// (every lane of the wave must be active in all four)
SX_HD void sx_agc_prefix_min(i32 (&v)[SX_AGC_PL]) {
    i32 x = v[0];
    x = sx_min(x, __builtin_amdgcn_update_dpp(x, x, 0x111, 0xF, 0xF, false));
    x = sx_min(x, __builtin_amdgcn_update_dpp(x, x, 0x112, 0xF, 0xF, false));
    x = sx_min(x, __builtin_amdgcn_update_dpp(x, x, 0x114, 0xF, 0xF, false));
    x = sx_min(x, __builtin_amdgcn_update_dpp(x, x, 0x118, 0xF, 0xF, false));
    x = sx_min(x, __builtin_amdgcn_update_dpp(x, x, 0x142, 0xA, 0xF, false));
    x = sx_min(x, __builtin_amdgcn_update_dpp(x, x, 0x143, 0xC, 0xF, false));
    v[0] = x;
}
// block b gets the value of block b + 1; block B - 1 keeps its own
SX_HD void sx_agc_from_next(const i32 (&v)[SX_AGC_PL], i32 (&o)[SX_AGC_PL], int B) {
    const i32 t = __shfl_down(v[0], 1, 64);
    o[0] = SX_LANE < B - 1 ? t : v[0];
}
// block b gets the value of block b - 1; block 0 gets `first`
SX_HD void sx_agc_from_prev(const i32 (&v)[SX_AGC_PL], i32 (&o)[SX_AGC_PL], i32 first) {
    const i32 t = __shfl_up(v[0], 1, 64);
    o[0] = SX_LANE > 0 ? t : first;
}
// the value of block b (wave-uniform), in every lane
SX_HD i32 sx_agc_at(const i32 (&v)[SX_AGC_PL], int b) { return __builtin_amdgcn_readlane(v[0], b); }
#else
SX_HD void sx_agc_prefix_min(i32 (&v)[SX_AGC_PL]) { for (int b = 1; b < SX_AGC_PL; b++) v[b] = sx_min(v[b], v[b - 1]); }
SX_HD void sx_agc_from_next(const i32 (&v)[SX_AGC_PL], i32 (&o)[SX_AGC_PL], int B) { for (int b = 0; b < SX_AGC_PL; b++) o[b] = b < B - 1 ? v[b + 1] : v[b]; }
SX_HD void sx_agc_from_prev(const i32 (&v)[SX_AGC_PL], i32 (&o)[SX_AGC_PL], i32 first) { for (int b = SX_AGC_PL - 1; b >= 0; b--) o[b] = b > 0 ? v[b - 1] : first; }
SX_HD i32 sx_agc_at(const i32 (&v)[SX_AGC_PL], int b) { return v[b]; }
#endif

struct alignas(16) SxAgcX8 { i16 s[8]; };                   // a 16-byte load: 8 samples; a block is four of them

struct SxAgcArgs {
    const i16* in; i16* out;        // [n][P][L]; out == in: in place
    i32* state;                     // [n_rows][SX_AGC_STATE_WORDS]
    const i32* map;                 // compact position -> row of the object, or NULL = the identity
    const u8* level_in; const u8* sa;       // [n][P] or NULL = the level of the input samples; [n][P][frames] or NULL = 255
    u8* level_out; i16* gain_out;   // [n][P] or NULL, both
    i32 n, n_packets, packet_samples, frames;
    SxAgcParams prm;
};

// row i of a call: what one wavefront does.  -> the row's packets with speech, and with some e_b < 32768, in every lane
SX_HD void sx_agc_row(const SxAgcArgs& a, int i, i32* n_speech, i32* n_limited) {
    const int P = a.n_packets, L = a.packet_samples, B = L >> 5;
    const SxAgcParams& q = a.prm;
    i32* const g = a.state + (size_t)(a.map ? SX_UNI(a.map[i]) : i) * SX_AGC_STATE_WORDS;
    i32 run = SX_UNI(g[0]), spl = SX_UNI(g[1]);
    i32 gain = sx_agc_clamp(SX_UNI(g[2]), -SX_AGC_MAX_GAIN_Q8, SX_AGC_MAX_GAIN_Q8);
    i32 glin = sx_agc_clamp(SX_UNI(g[3]), 0, T_agc_db[60]);
    i32 env = sx_agc_clamp(SX_UNI(g[4]), 0, SX_AGC_ONE_Q15);
    i32 speech_packets = 0, limited_packets = 0;
    for (int p = 0; p < P; p++) {
        const size_t at = (size_t)i * P + p;
        const SxAgcX8* src = (const SxAgcX8*)(a.in + at * (size_t)L);
        SxAgcX8* dst = (SxAgcX8*)(a.out + at * (size_t)L);
        // the packet: block b as four 16-byte loads, held until the store
        SxAgcX8 x[SX_AGC_PL][4];
        i64 e_in = 0;
#pragma unroll
        for (int k = 0; k < SX_AGC_PL; k++) {
            const int b = SX_LANE + k * SX_NLANES;
            if (b < B) {
#pragma unroll
                for (int c = 0; c < 4; c++) x[k][c] = src[4 * b + c];
                if (!a.level_in) {
#pragma unroll
                    for (int s = 0; s < 32; s++) { const i32 v = x[k][s >> 3].s[s & 7]; e_in += (i64)(v * v); }
                }
            }
        }
        // 1. observation
        const i32 lv = a.level_in ? sx_min(SX_UNI(a.level_in[at]), 127) : sx_vad_level(wv_sum64(e_in), L);
        i32 act = 255;
        if (a.sa) {
            act = 0;
            SX_PAR(f, a.frames) act = sx_max(act, (i32)a.sa[at * (size_t)a.frames + f]);
            act = wv_max(act);
        }
        const bool speech = act >= q.sa_on_q8 && lv <= q.gate_level;
        // 2. level and gain (the differences in 64 bits: spl is whatever the record held)
        if (speech) {
            speech_packets++;
            if (run == 0) { spl = lv << 8; run = 1; }
            else spl = (i32)((i64)spl + ((((i64)(lv << 8) - (i64)spl) * q.alpha_q8) >> 8));
            const i32 want = (i32)sx_agc_clamp64((i64)spl - (q.target_level << 8), -(q.max_cut_db << 8), q.max_boost_db << 8);
            gain += sx_agc_clamp(want - gain, -q.slew_down_q8, q.slew_up_q8);
        }
        // 3. the gain, with a ramp over the first 256 samples; the block's peak
        const i32 g0 = glin, dg = sx_agc_lin(gain) - g0;
        glin = g0 + dg;
        i32 y0[SX_AGC_PL][32], ab[SX_AGC_PL];
#pragma unroll
        for (int k = 0; k < SX_AGC_PL; k++) {
            const int b = SX_LANE + k * SX_NLANES;
            i32 pk = 0;
            if (b < B) {
#pragma unroll
                for (int s = 0; s < 32; s++) {
                    const i32 gs = g0 + ((dg * sx_min(32 * b + s + 1, 256)) >> 8);
                    const i32 v = (i32)(((i64)x[k][s >> 3].s[s & 7] * (i64)gs + 32768) >> 16);
                    y0[k][s] = v;
                    pk = sx_max(pk, v < 0 ? -v : v);
                }
            }
            // 4. the limiter: the block's attenuation ...
            ab[k] = pk <= q.ceiling ? SX_AGC_ONE_Q15 : (i32)(((u32)q.ceiling << 15) / (u32)pk);
        }
        // ... one block of look-ahead, and the envelope in its closed form
        i32 an[SX_AGC_PL], m[SX_AGC_PL], e[SX_AGC_PL], ep[SX_AGC_PL];
        sx_agc_from_next(ab, an, B);
        const i32 rel = q.release_q15;
        const i32 e_first = sx_min(env, sx_agc_at(ab, 0));
#pragma unroll
        for (int k = 0; k < SX_AGC_PL; k++) m[k] = sx_min(ab[k], an[k]) - (SX_LANE + k * SX_NLANES) * rel;
        sx_agc_prefix_min(m);
        i32 limited = 0;
#pragma unroll
        for (int k = 0; k < SX_AGC_PL; k++) {
            const int b = SX_LANE + k * SX_NLANES;
            e[k] = b * rel + sx_min(e_first + rel, m[k]);
            if (b < B && e[k] < SX_AGC_ONE_Q15) limited = 1;
        }
        sx_agc_from_prev(e, ep, e_first);
        env = sx_agc_at(e, B - 1);
        limited_packets += wv_max(limited);
        // 5. output
        i64 e_out = 0;
#pragma unroll
        for (int k = 0; k < SX_AGC_PL; k++) {
            const int b = SX_LANE + k * SX_NLANES;
            if (b < B) {
                const i32 de = e[k] - ep[k];
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    SxAgcX8 o;
#pragma unroll
                    for (int s = 0; s < 8; s++) {
                        const i32 es = ep[k] + ((de * (8 * c + s + 1)) >> 5);
                        const i32 y = (i32)(((i64)y0[k][8 * c + s] * (i64)es + 16384) >> 15);
                        o.s[s] = (i16)y;
                        e_out += (i64)(y * y);
                    }
                    dst[4 * b + c] = o;
                }
            }
        }
        // 6. reports
        if (a.level_out) {
            const i32 lo = sx_vad_level(wv_sum64(e_out), L);
            if (SX_LANE == 0) a.level_out[at] = (u8)lo;
        }
        if (a.gain_out && SX_LANE == 0) a.gain_out[at] = (i16)gain;
    }
    if (SX_LANE == 0) { g[0] = run; g[1] = spl; g[2] = gain; g[3] = glin; g[4] = env; }
    *n_speech = speech_packets; *n_limited = limited_packets;
}

#if defined(__HIPCC__)
// The count of a call without a second kernel and without a fence.  The object owns one 64-bit word per group of 32 rows of a call and
// a root word, each on a 128-byte line of its own and zero between calls.  A row adds {1, its speech packets, its limited packets} to its
// group's word with ONE atomic; the value that atomic returns tells the row that it is the group's last and, with its own addend, what
// the group counted.  That row clears the word and adds {1, the group's counts} to the root the same way, and the group that finds
// itself last there writes d_count and clears the root.  Every word is its own total order, the sums travel in the returned values, so
// nothing has to be ordered between two addresses; a group's 32 atomics and the root's n / 32 are all that meet on one address (one
// atomic per row on a single word was measured first: 0.12 ms at 4096 rows, against 0.04 ms for solo_vad).
// Fields, ticket on top so that its last carry leaves the word: group = rows done (6 bits) | limited (29) | speech (29), a group's counts
// being < 32 P < 2^28; root = groups done (18) | limited (23) | speech (23), as n P < 2^23 and n / 32 <= 2^18.
#define SX_AGC_GROUP 32
#define SX_AGC_ACC_STRIDE 16                                // 64-bit words between two counters: 128 bytes
static inline size_t solo_agc_acc_bytes(int n_rows) { return ((size_t)(n_rows + SX_AGC_GROUP - 1) / SX_AGC_GROUP + 1) * SX_AGC_ACC_STRIDE * sizeof(u64); }

// One wavefront per row of the call
__global__ void __launch_bounds__(64) solo_agc_kernel(const SxAgcArgs a, SxAgcCount* count, unsigned long long* acc, const u32* verdict) {
    if (sx_map_refused(a.map, verdict)) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && count) count->rows = -1;
        return;
    }
    i32 speech, limited;
    sx_agc_row(a, (int)blockIdx.x, &speech, &limited);
    if (count && threadIdx.x == 0) {
        const u32 grp = blockIdx.x / SX_AGC_GROUP, n_groups = ((u32)a.n + SX_AGC_GROUP - 1) / SX_AGC_GROUP;
        const u32 size = grp == n_groups - 1 ? (u32)a.n - grp * SX_AGC_GROUP : SX_AGC_GROUP;
        unsigned long long* const gw = acc + (size_t)(grp + 1) * SX_AGC_ACC_STRIDE;
        const u64 mine = (u64)(u32)speech | ((u64)(u32)limited << 29) | ((u64)1 << 58);
        const u64 seen = atomicAdd(gw, (unsigned long long)mine);
        if ((u32)(seen >> 58) == size - 1) {
            const u64 tot = seen + mine;
            atomicExch(gw, 0ull);
            const u64 up = (tot & 0x1FFFFFFF) | (((tot >> 29) & 0x1FFFFFFF) << 23) | ((u64)1 << 46);
            const u64 root = atomicAdd(acc, (unsigned long long)up);
            if ((u32)(root >> 46) == n_groups - 1) {
                const u64 all = root + up;
                atomicExch(acc, 0ull);
                SxAgcCount c;
                c.rows = a.n; c.speech = (i32)(all & 0x7FFFFF); c.limited = (i32)((all >> 23) & 0x7FFFFF); c.zero = 0;
                *count = c;
            }
        }
    }
}
static inline hipError_t solo_agc_launch(const SxAgcArgs& a, SxAgcCount* count, unsigned long long* acc, const u32* verdict, hipStream_t s) {
    hipLaunchKernelGGL(solo_agc_kernel, dim3((unsigned)a.n), dim3(64), 0, s, a, count, acc, verdict);
    return hipGetLastError();
}
#else
// Host form of the launch (tests): every row through sx_agc_row.  -> false: the list is not strictly increasing inside [0, n_rows),
// nothing but count->rows = -1 is written
static inline bool sx_agc_host(const SxAgcArgs& a, int n_rows, SxAgcCount* count) {
    if (!sx_map_ok(a.map, a.n, n_rows)) {
        if (count) count->rows = -1;
        return false;
    }
    SxAgcCount c; c.rows = a.n; c.speech = 0; c.limited = 0; c.zero = 0;
    for (int i = 0; i < a.n; i++) {
        i32 s, l;
        sx_agc_row(a, i, &s, &l);
        c.speech += s; c.limited += l;
    }
    if (count) *count = c;
    return true;
}
#endif

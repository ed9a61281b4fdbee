// solo_timescale.h -- play-out time scaling between play-out and mix: `a` decoded packets of a row -> `b` packets of audio without a click
// (solo_timescale, include/solo_mi355x.h, whose comment is the reference for the arithmetic).  Waveform-similarity overlap-add on int16
// rows in integer arithmetic, per row and stateless: the output is cut into M = Lo / H blocks of H = 5 ms; block m is taken from the input
// near its nominal position n_m, at the lag d in [-D, D] (D = 3H / 2, clipped to the row) whose H samples are closest -- least sum of
// absolute differences, then least |d|, then negative before positive -- to what the previous block's segment would have played next (the
// template), and is cross-faded with that template over its H samples.  The first block is the input's first H samples, the last one is
// pinned to the input's last H, and the block before the last also counts how well ITS continuation meets that pinned end.
//
// The cut: ONE wavefront per row.
//   * stage    the row's Li <= 5120 samples go to LDS by 16-byte loads, as unsigned numbers (x ^ 0x8000: |a - b| is unchanged), two to a
//              dword as they lie in memory
//   * search   the M - 2 searched blocks are a serial chain (block m's template starts where block m - 1 was cut).  Per block the lanes
//              own contiguous runs of R = H / 20 lags (4 at H = 80, 8 at H = 160: 64 R >= 3H + 1 candidates).  The windows of a lane's
//              lags share all but R - 1 samples: the lane reads its H + R samples once, as aligned dwords A[i], forms the odd-aligned
//              pairs B[i] = (A[i].hi, A[i + 1].lo) with one v_alignbit each, and every dword of the template (wave-uniform, a broadcast
//              read) then meets R + 1 of them in ONE instruction per lag: v_sad_u16 adds both halves' absolute differences to the lag's
//              32-bit sum, which stays in a register.  R + 1, not R: whether a lane's first sample is the low or the high half of its
//              dword (`par`, wave-uniform because R is even) shifts the lags by one against the A / B grid; the sums are taken for the
//              grid positions 0 .. R and lag r reads position r + par.  One wave-wide arg-min of (cost, rank) per block (wv_argmin).
//   * fade     once every cut is known the cross-fades are independent: lane l owns 8 output samples at a time, one 16-byte store each.
// No scratch, no atomics on PCM; the row's costs go to the call's count with one 64-bit atomic per wavefront (integer: any order).
//
// Everything outside the kernels compiles for the host as well (tests/test_timescale_model.py builds sx_ts_host: the rows run through the
// very functions of the kernel, with the 1-lane forms of solo_wave.h, and are compared with an independent model).
#pragma once
#include "solo_wave.h"
#include "../../include/solo_mi355x.h"

#define SX_TS_MAX_PACKETS 4
#define SX_TS_MAX_L 1280                                    // samples of the longest packet (40 ms at 32 kHz)
#define SX_TS_PAD 16                                        // samples kept (zero) behind the row in LDS: a lane whose run of lags crosses the last
                                                            // candidate, and the template's pairing, read up to R + 1 samples past the row
#define SX_TS_MAX_BLOCKS 32                                 // 4 packets of 8 blocks

typedef solo_timescale_count_t SxTsCount;
static_assert(sizeof(SxTsCount) == 16, "solo_timescale_count_t layout");

struct alignas(16) SxTsX8 { u32 d[4]; };                    // what one lane loads and stores: 8 samples

struct SxTsArgs {
    const i16* pcm_in; i16* pcm_out;
    i32* shift; i32* cost;                                  // [n][M] or NULL
    int Li, Lo, H;                                          // samples of an input row, of an output row, of a block
};

// LDS of a row (bytes; every part a multiple of 16): the samples and their pad | s_m, d_m and cost_m of every block
SX_HD int sx_ts_row_words(int Li) { return (Li + SX_TS_PAD) >> 1; }
SX_HD size_t sx_ts_lds_bytes(int Li) { return (size_t)sx_ts_row_words(Li) * 4 + 3 * SX_TS_MAX_BLOCKS * sizeof(i32); }

// |a.lo - b.lo| + |a.hi - b.hi| + c, the halves as unsigned 16-bit numbers
SX_HD u32 sx_ts_sad(u32 a, u32 b, u32 c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u16(a, b, c);
#else
    const i32 l = (i32)(a & 0xFFFFu) - (i32)(b & 0xFFFFu), h = (i32)(a >> 16) - (i32)(b >> 16);
    return c + (u32)(l < 0 ? -l : l) + (u32)(h < 0 ? -h : h);
#endif
}
// (lo.hi, hi.lo): the pair of samples that straddles two dwords
SX_HD u32 sx_ts_straddle(u32 hi, u32 lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, 16);
#else
    return (lo >> 16) | (hi << 16);
#endif
}
// the samples (pos + 2i, pos + 2i + 1) of the row as one dword
SX_HD u32 sx_ts_pair(const u32* X, int pos, int i) {
    const int q = (pos >> 1) + i;
    const u32 lo = X[q];
    return (pos & 1) ? sx_ts_straddle(X[q + 1], lo) : lo;
}
// the nominal source position of block m
SX_HD int sx_ts_nominal(int m, int Li, int H, int M) { return (2 * m * (Li - H) + (M - 1)) / (2 * (M - 1)); }
// the order among equal costs: |d| first, then the negative lag
SX_HD i32 sx_ts_rank(int d) { return d < 0 ? -2 * d - 1 : 2 * d; }
SX_HD int sx_ts_unrank(i32 r) { return (r & 1) ? -((r + 1) >> 1) : (r >> 1); }

// acc[p] += sum_j |x[tpos + j] - x[2 (base >> 1) + p + j]|, p = 0 .. R: the template at sample tpos against this lane's R + 1 grid positions
template <int H, int R>
SX_HD void sx_ts_sads(const u32* X, int tpos, int base, u32 (&acc)[R + 1]) {
    const int q = base >> 1, tq = tpos >> 1;
    const bool todd = tpos & 1;                             // wave-uniform
    for (int j0 = 0; j0 < H / 2; j0 += 8) {
        u32 A[8 + R / 2], B[7 + R / 2], Tr[9], T[8];
#pragma unroll
        for (int i = 0; i < 8 + R / 2; i++) A[i] = X[q + j0 + i];
#pragma unroll
        for (int i = 0; i < 9; i++) Tr[i] = X[tq + j0 + i];
#pragma unroll
        for (int i = 0; i < 7 + R / 2; i++) B[i] = sx_ts_straddle(A[i + 1], A[i]);
#pragma unroll
        for (int i = 0; i < 8; i++) T[i] = todd ? sx_ts_straddle(Tr[i + 1], Tr[i]) : Tr[i];
#pragma unroll
        for (int jj = 0; jj < 8; jj++)
#pragma unroll
            for (int p = 0; p <= R; p++) acc[p] = sx_ts_sad((p & 1) ? B[jj + (p >> 1)] : A[jj + (p >> 1)], T[jj], acc[p]);
    }
}

// One row: what one wavefront does.  lds: sx_ts_lds_bytes(a.Li) bytes, 16-byte aligned.  -> the sum of the row's splice costs (the wave's,
// in every lane)
template <int H>
SX_HD i64 sx_ts_row(const SxTsArgs& a, int row, u32* lds) {
    constexpr int R = H / 20, D = 3 * H / 2;
    static_assert(R % 2 == 0 && 64 * R >= 2 * D + 1 && H % 16 == 0, "lags per lane");
    const int Li = a.Li, Lo = a.Lo, M = Lo / H;
    u32* X = lds;
    i32* s_of = (i32*)(lds + sx_ts_row_words(Li));
    i32* d_of = s_of + SX_TS_MAX_BLOCKS;
    i32* c_of = d_of + SX_TS_MAX_BLOCKS;

    // stage: 8 samples per lane and step, biased to unsigned; the pad behind the row is zero
    const SxTsX8* in = (const SxTsX8*)(a.pcm_in + (size_t)row * (size_t)Li);
    SX_PAR(ch, (Li + SX_TS_PAD) >> 3) {
        SxTsX8 v;
        if (ch < (Li >> 3)) {
            v = in[ch];
#pragma unroll
            for (int k = 0; k < 4; k++) v.d[k] ^= 0x80008000u;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) v.d[k] = 0;
        }
        ((SxTsX8*)X)[ch] = v;
    }
    if (SX_LANE == 0) { s_of[0] = 0; d_of[0] = 0; c_of[0] = 0; }
    wv_sync();

    // search: the chain of cuts
    int s_prev = 0;
    i64 total = 0;
    for (int m = 1; m < M - 1; m++) {
        const int nm = sx_ts_nominal(m, Li, H, M), tpos = s_prev + H;
        const int lo = sx_max(-D, -nm), hi = sx_min(D, Li - 2 * H - nm), ncand = hi - lo + 1, w0 = nm + lo;
        const u32 pmask = 0u - (u32)(w0 & 1);              // par: all ones when the lanes' first sample is the high half of its dword
        i32 bc = 0x7FFFFFFF, br = 0x7FFFFFFF;
        for (int c0 = SX_LANE * R; c0 < ncand; c0 += SX_NLANES * R) {      // (one trip on the device: 64 R >= 2 D + 1)
            u32 acc[R + 1];
#pragma unroll
            for (int p = 0; p <= R; p++) acc[p] = 0;
            sx_ts_sads<H, R>(X, tpos, w0 + c0, acc);
            if (m == M - 2) sx_ts_sads<H, R>(X, Li - H, w0 + c0 + H, acc);  // how the candidate's continuation meets the pinned last block
#pragma unroll
            for (int r = 0; r < R; r++) {
                const i32 c = (i32)((acc[r] & ~pmask) | (acc[r + 1] & pmask)), rk = sx_ts_rank(lo + c0 + r);      // acc[r + par], kept in registers
                if (c0 + r < ncand && (c < bc || (c == bc && rk < br))) { bc = c; br = rk; }
            }
        }
        wv_argmin(&bc, &br);
        bc = SX_UNI(bc); br = SX_UNI(br);
        const int d = sx_ts_unrank(br);
        s_prev = nm + d;
        total += bc;
        if (SX_LANE == 0) { s_of[m] = s_prev; d_of[m] = d; c_of[m] = bc; }
    }
    {   // the last block: pinned to the row's end
        i32 c = 0;
        SX_PAR(jj, H / 2) c = (i32)sx_ts_sad(sx_ts_pair(X, s_prev + H, jj), X[((Li - H) >> 1) + jj], (u32)c);
        c = wv_sum(c);
        total += c;
        if (SX_LANE == 0) { s_of[M - 1] = Li - H; d_of[M - 1] = 0; c_of[M - 1] = c; }
    }
    wv_sync();

    // fade: y[mH + j] = floor((t[j] (H - 1 - j) + x[s_m + j] (j + 1) + H / 2) / H); block 0 fades the row's start into itself.  On the
    // biased numbers the quotient is the biased result (H x 32768 leaves the numerator), and nothing is negative
    const u16* xs = (const u16*)X;
    SxTsX8* out = (SxTsX8*)(a.pcm_out + (size_t)row * (size_t)Lo);
    SX_PAR(ch, Lo >> 3) {
        const int m = ch / (H / 8), j0 = (ch - m * (H / 8)) * 8;
        const int sm = s_of[m], tp = m ? s_of[m - 1] + H : 0;
        SxTsX8 v;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            u32 y[2];
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const int j = j0 + 2 * k + e;
                y[e] = ((u32)xs[tp + j] * (u32)(H - 1 - j) + (u32)xs[sm + j] * (u32)(j + 1) + (u32)(H / 2)) / (u32)H;
            }
            v.d[k] = (y[0] | (y[1] << 16)) ^ 0x80008000u;
        }
        out[ch] = v;
    }
    if (a.shift) SX_PAR(m, M) a.shift[(size_t)row * M + m] = d_of[m];
    if (a.cost) SX_PAR(m, M) a.cost[(size_t)row * M + m] = c_of[m];
    return total;
}
SX_HD i64 sx_ts_row_any(const SxTsArgs& a, int row, u32* lds) { return a.H == 80 ? sx_ts_row<80>(a, row, lds) : sx_ts_row<160>(a, row, lds); }

// what the call refuses before anything is enqueued (fs, L: the handle's sample rate and packet samples)
static inline bool sx_ts_args_ok(const void* pcm_in, long long n, int in_packets, int out_packets, int fs, int L, const void* pcm_out) {
    if (!pcm_in || !pcm_out || n <= 0) return false;
    if (in_packets < 1 || in_packets > SX_TS_MAX_PACKETS || out_packets < 1 || out_packets > SX_TS_MAX_PACKETS) return false;
    const int H = fs / 200;
    if ((H != 80 && H != 160) || L <= 0 || L > SX_TS_MAX_L || L % H) return false;
    if (n * (long long)sx_max(in_packets, out_packets) * (long long)L >= (1LL << 31)) return false;
    const uintptr_t in0 = (uintptr_t)pcm_in, out0 = (uintptr_t)pcm_out;
    const uintptr_t in_bytes = (uintptr_t)n * (uintptr_t)in_packets * (uintptr_t)L * sizeof(i16);
    const uintptr_t out_bytes = (uintptr_t)n * (uintptr_t)out_packets * (uintptr_t)L * sizeof(i16);
    return !(in0 & 15) && !(out0 & 15) && !(in0 < out0 + out_bytes && out0 < in0 + in_bytes);
}
// blocks of a row that are searched
static inline int sx_ts_searched(int Lo, int H) { return Lo / H - 2; }

#if defined(__HIPCC__)
// the count before the rows add their costs (one lane)
__global__ void __launch_bounds__(64) solo_timescale_count_kernel(SxTsCount* count, i32 rows, i32 blocks) {
    if (threadIdx.x == 0) { SxTsCount c; c.rows = rows; c.blocks = blocks; c.cost = 0; *count = c; }
}
// one wavefront per row
__global__ void __launch_bounds__(64) solo_timescale_kernel(const SxTsArgs a, SxTsCount* count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sx_ts_lds[];
    const i64 cost = sx_ts_row_any(a, (int)blockIdx.x, (u32*)sx_ts_lds);
    if (threadIdx.x == 0 && count && cost) atomicAdd((unsigned long long*)&count->cost, (unsigned long long)cost);
}
static inline hipError_t solo_timescale_launch(const SxTsArgs& a, int n, SxTsCount* count, hipStream_t s) {
    if (count) hipLaunchKernelGGL(solo_timescale_count_kernel, dim3(1), dim3(64), 0, s, count, n, n * sx_ts_searched(a.Lo, a.H));
    hipLaunchKernelGGL(solo_timescale_kernel, dim3((unsigned)n), dim3(64), sx_ts_lds_bytes(a.Li), s, a, count);
    return hipGetLastError();
}
#else
// Host form of the launch (tests): every row through sx_ts_row
static inline void sx_ts_host(const SxTsArgs& a, int n, SxTsCount* count) {
    SxTsX8* lds = new SxTsX8[(sx_ts_lds_bytes(a.Li) + 15) / 16];
    i64 cost = 0;
    for (int row = 0; row < n; row++) cost += sx_ts_row_any(a, row, (u32*)lds);
    if (count) { count->rows = n; count->blocks = n * sx_ts_searched(a.Lo, a.H); count->cost = cost; }
    delete[] lds;
}
#endif

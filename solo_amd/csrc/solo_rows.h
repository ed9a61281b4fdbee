// solo_rows.h -- the record kernels of the row-state objects (solo_resample_*, solo_vad_*, solo_agc_*, solo_playout_*; the objects
// themselves: solo_rows of solo_api.hip).  An object keeps one state record of `words` 32-bit words per row, state [n_rows][words],
// and optionally a second segment per row, extra [n_rows][extra_words] (Playout's held packet: packet_samples / 2 words); without
// one, extra = NULL and extra_words = 0.  Rate-independent and stage-independent: compiled once, the record a reset leaves is data.
#pragma once
#include "solo_wave.h"
#include "solo_stream_ctl.h"

#define SX_ROWS_MAX_WORDS 32
struct SxRowInit { i32 w[SX_ROWS_MAX_WORDS]; };             // the record a reset leaves (the second segment: zeros); travels by value

#if defined(__HIPCC__)
// the listed rows back to the initial state: one wavefront per row, the list travels by value (solo_stream_ctl.h)
__global__ void __launch_bounds__(64) solo_rows_reset_kernel(i32* state, int words, const SxRowInit init, i32* extra, int extra_words, const SxStreamCtlList l) {
    const int row = l.r[blockIdx.x].stream;
    if ((int)threadIdx.x < words) state[(size_t)row * words + threadIdx.x] = init.w[threadIdx.x];
    i32* x = extra + (size_t)row * extra_words;
    SX_PAR(w, extra_words) x[w] = 0;
}
// every row: one lane per word
__global__ void __launch_bounds__(256) solo_rows_reset_all_kernel(i32* state, int words, const SxRowInit init, i32* extra, int extra_words, int n_rows) {
    const size_t rw = (size_t)words + extra_words, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n_rows * rw) return;
    const size_t row = i / rw;
    const int w = (int)(i % rw);
    if (w < words) state[row * words + w] = init.w[w];
    else extra[row * extra_words + (w - words)] = 0;
}
// plain copies of the listed rows (rows = NULL: rows 0 .. n - 1) to (put = 0) or from a blob of words + extra_words words a row: the
// record, then the second segment; an index outside [0, n_rows) moves nothing
__global__ void __launch_bounds__(256) solo_rows_copy_kernel(i32* state, int words, i32* extra, int extra_words, int n_rows, const i32* rows, int n, i32* blob,
                                                             int put) {
    const size_t rw = (size_t)words + extra_words, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * rw) return;
    const int r = (int)(i / rw), w = (int)(i % rw);
    const int row = rows ? rows[r] : r;
    if (row < 0 || row >= n_rows) return;
    i32* s = w < words ? state + (size_t)row * words + w : extra + (size_t)row * extra_words + (w - words);
    if (put) *s = blob[i];
    else blob[i] = *s;
}
#endif

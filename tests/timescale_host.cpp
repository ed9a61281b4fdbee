// Host build of the play-out time scaler (solo_amd/csrc/solo_timescale.h) for tests/test_timescale_model.py, which compiles this file
// into a temporary directory through tests/host_build.py.
#include <string.h>
#include "../solo_amd/csrc/solo_timescale.h"

extern "C" {

int emu_ts_count_size() { return (int)sizeof(SxTsCount); }
int emu_ts_lds_bytes(int Li) { return (int)sx_ts_lds_bytes(Li); }
int emu_ts_nominal(int m, int Li, int H, int M) { return sx_ts_nominal(m, Li, H, M); }
int emu_ts_rank(int d) { return sx_ts_rank(d); }
int emu_ts_unrank(int r) { return sx_ts_unrank(r); }
unsigned emu_ts_sad(unsigned a, unsigned b, unsigned c) { return sx_ts_sad(a, b, c); }
unsigned emu_ts_straddle(unsigned hi, unsigned lo) { return sx_ts_straddle(hi, lo); }

// -> 0, or -1 when the call is refused (nothing written)
int emu_timescale(const short* pcm_in, int n, int in_packets, int out_packets, int fs, int L, short* pcm_out, int* shift, int* cost, void* count) {
    if (!sx_ts_args_ok(pcm_in, n, in_packets, out_packets, fs, L, pcm_out)) return -1;
    SxTsArgs a;
    a.pcm_in = pcm_in; a.pcm_out = pcm_out; a.shift = shift; a.cost = cost;
    a.Li = in_packets * L; a.Lo = out_packets * L; a.H = fs / 200;
    sx_ts_host(a, n, (SxTsCount*)count);
    return 0;
}

}

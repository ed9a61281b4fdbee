// Host build of the PCM resampler (solo_amd/csrc/solo_resample.h) for tests/test_resample_model.py, which compiles this file into a
// temporary directory through tests/host_build.py.
#include <string.h>
#include "../solo_amd/csrc/solo_resample.h"

extern "C" {

int emu_rs_rows_per_group() { return SX_RS_ROWS; }
int emu_rs_state_bytes() { return SX_RS_STATE_WORDS * 4; }
int emu_rs_count_size() { return (int)sizeof(SxRsCount); }

// -> 1 when the library offers the pair
int emu_rs_supported(int fs_in, int fs_out) { SxRsCfg c; return sx_rs_config(fs_in, fs_out, &c) ? 1 : 0; }
int emu_rs_out_samples(int fs_in, int fs_out, int in_samples) {
    SxRsCfg c;
    return sx_rs_config(fs_in, fs_out, &c) ? sx_rs_out_samples(c, in_samples) : -1;
}
// the host's checks of a call (solo_resample / solo_resample_rows) -> 1 = accepted
int emu_rs_call_ok(int fs_in, int fs_out, int n_rows, int n, int n_packets, int in_samples, const void* in, const void* out) {
    SxRsCfg c;
    return sx_rs_config(fs_in, fs_out, &c) && sx_rs_call_ok(c, n_rows, n, n_packets, in_samples, in, out) ? 1 : 0;
}
int emu_rs_list_ok(const int* rows, int n, int n_rows) { return sx_rs_list_ok(rows, n, n_rows) ? 1 : 0; }

// state: int32 [n_rows][24], carried by the caller; map: NULL or n row indices.  -> 0, -1 = refused by the host's checks,
// -2 = the list was refused (count->rows = -1, nothing else written)
int emu_rs_run(int fs_in, int fs_out, int n_rows, int* state, const int* map, int n, const short* in, int n_packets, int in_samples, short* out,
               void* count) {
    SxRsArgs a;
    if (!sx_rs_config(fs_in, fs_out, &a.c) || !sx_rs_call_ok(a.c, n_rows, n, n_packets, in_samples, in, out)) return -1;
    a.in = in; a.out = out; a.state = state; a.map = map; a.n = n;
    a.batches = n_packets * (in_samples / a.c.n_in);
    return sx_rs_host(a, n_rows, (SxRsCount*)count) ? 0 : -2;
}

}

// Host build of the level control stage (solo_amd/csrc/solo_agc.h) for tests/test_agc_model.py and tests/test_agc_abi.py, which compile
// this file into a temporary directory through tests/host_build.py.
#include <string.h>
#include "../solo_amd/csrc/solo_agc.h"

extern "C" {

int emu_agc_state_bytes() { return SX_AGC_STATE_WORDS * 4; }
int emu_agc_count_size() { return (int)sizeof(SxAgcCount); }
int emu_agc_params_size() { return (int)sizeof(SxAgcParams); }
int emu_agc_table_db(int i) { return T_agc_db[i]; }
int emu_agc_table_frac(int r) { return T_agc_frac[r]; }
int emu_agc_lin(int d) { return sx_agc_lin(d); }
// the six steps of the 64-lane prefix minimum on 64 values
void emu_agc_prefix_min_steps(int* v) { sx_agc_prefix_min_steps(v); }

// the record the create and reset calls leave: 16 words
void emu_agc_init(int* state, int n_rows) {
    for (int r = 0; r < n_rows; r++)
        for (int w = 0; w < SX_AGC_STATE_WORDS; w++) state[r * SX_AGC_STATE_WORDS + w] = sx_agc_init_word(w);
}

// the host's checks of the call -> 1 = accepted
int emu_agc_call_ok(int n_rows, const void* rows, int n, const void* pcm_in, int n_packets, int packet_samples, const void* sa, int frames, const int* params,
                    const void* pcm_out, const void* count) {
    return sx_agc_call_ok(n_rows, rows, n, pcm_in, n_packets, packet_samples, sa, frames, (const SxAgcParams*)params, pcm_out, count) ? 1 : 0;
}
int emu_agc_list_ok(const int* rows, int n, int n_rows) { return sx_vad_list_ok(rows, n, n_rows) ? 1 : 0; }

// state: int32 [n_rows][16], carried by the caller; map: NULL or n row indices.  -> 0, -1 = refused by the host's checks, -2 = the list
// was refused (count->rows = -1, nothing else written)
int emu_agc_run(int n_rows, int* state, const int* map, int n, const short* pcm_in, int n_packets, int packet_samples, const unsigned char* level_in,
                const unsigned char* sa, int frames, const int* params, short* pcm_out, unsigned char* level_out, short* gain_out, void* count) {
    if (!sx_agc_call_ok(n_rows, map, n, pcm_in, n_packets, packet_samples, sa, frames, (const SxAgcParams*)params, pcm_out, count)) return -1;
    SxAgcArgs a;
    a.in = pcm_in; a.out = pcm_out; a.state = state; a.map = map; a.level_in = level_in; a.sa = sa; a.level_out = level_out; a.gain_out = gain_out;
    a.n = n; a.n_packets = n_packets; a.packet_samples = packet_samples; a.frames = sa ? frames : 0; a.prm = *(const SxAgcParams*)params;
    return sx_agc_host(a, n_rows, (SxAgcCount*)count) ? 0 : -2;
}

}

// Host build of the VAD stage (solo_amd/csrc/solo_vad.h) for tests/test_vad_model.py and tests/test_vad_abi.py, which compile this file
// into a temporary directory through tests/host_build.py.
#include <string.h>
#include "../solo_amd/csrc/solo_vad.h"

extern "C" {

int emu_vad_state_bytes() { return SX_VAD_STATE_WORDS * 4; }
int emu_vad_count_size() { return (int)sizeof(SxVadCount); }
int emu_vad_params_size() { return (int)sizeof(SxVadSelectParams); }
int emu_vad_frame_ok(int frame) { return sx_vad_frame_ok(frame) ? 1 : 0; }
unsigned long long emu_vad_threshold(int k) { return T_vad_level[k]; }
int emu_vad_level(long long E, int packet_samples) { return sx_vad_level(E, packet_samples); }

// the record the create and reset calls leave: 32 words
void emu_vad_init(int* state, int n_rows) {
    for (int r = 0; r < n_rows; r++)
        for (int w = 0; w < SX_VAD_STATE_WORDS; w++) state[r * SX_VAD_STATE_WORDS + w] = sx_vad_init_word(w);
}

// the host's checks of the calls -> 1 = accepted
int emu_vad_call_ok(int frame, int n_rows, const void* rows, int n, const void* pcm, int n_packets, int packet_samples, const void* sa, const void* count) {
    return sx_vad_call_ok(frame, n_rows, rows, n, pcm, n_packets, packet_samples, sa, count) ? 1 : 0;
}
int emu_vsel_call_ok(int n_rows, int n, const void* sa, const void* level, int n_packets, int frames, const void* room, int n_rooms, const int* params,
                     const void* sel, const void* count) {
    return sx_vsel_call_ok(n_rows, n, sa, level, n_packets, frames, room, n_rooms, (const SxVadSelectParams*)params, sel, count) ? 1 : 0;
}
int emu_vad_list_ok(const int* rows, int n, int n_rows) { return sx_vad_list_ok(rows, n, n_rows) ? 1 : 0; }

// state: int32 [n_rows][32], carried by the caller; map: NULL or n row indices.  -> 0, -1 = refused by the host's checks, -2 = the list
// was refused (count->rows = -1, nothing else written)
int emu_vad_run(int frame, int n_rows, int* state, const int* map, int n, const short* pcm, int n_packets, int packet_samples, unsigned char* sa,
                int* detail, unsigned char* level, void* count) {
    if (!sx_vad_call_ok(frame, n_rows, map, n, pcm, n_packets, packet_samples, sa, count)) return -1;
    SxVadArgs a;
    a.pcm = pcm; a.state = state; a.map = map; a.sa = sa; a.detail = detail; a.level = level;
    a.n = n; a.n_packets = n_packets; a.packet_samples = packet_samples;
    return sx_vad_host(frame, a, n_rows, (SxVadCount*)count) ? 0 : -2;
}
int emu_vsel_run(int n_rows, int* state, const int* map, int n, const unsigned char* sa, const unsigned char* level, int n_packets, int frames,
                 const int* room, int n_rooms, const int* params, const short* gain_in, unsigned char* sel, short* gain_out, unsigned char* keep,
                 int* dominant, void* count) {
    if (!sx_vsel_call_ok(n_rows, n, sa, level, n_packets, frames, room, n_rooms, (const SxVadSelectParams*)params, sel, count)) return -1;
    SxVselArgs a;
    memset(&a, 0, sizeof(a));
    a.sa = sa; a.level = level; a.gain_in = gain_in; a.map = map; a.sel = sel; a.gain_out = gain_out; a.keep = keep; a.dominant = dominant;
    a.state = state; a.n_packets = n_packets; a.frames = frames; a.prm = *(const SxVadSelectParams*)params;
    return sx_vsel_host(a, room, n, n_rooms, n_rows, (SxVadCount*)count) ? 0 : -2;
}

}

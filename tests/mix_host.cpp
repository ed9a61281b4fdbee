// Host build of the mixing bridge (solo_amd/csrc/solo_mix.h) for tests/test_mix_model.py, which compiles this file into a temporary
// directory through tests/host_build.py.
#include <string.h>
#include "../solo_amd/csrc/solo_mix.h"

extern "C" {

int emu_mix_count_size() { return (int)sizeof(SxMixCount); }
int emu_mix_cache_rows(int L) { return SX_MIX_CACHE_CHUNKS / (L / 8); }

// -> 0, or -1 when a room id was refused (count->rows = -1, nothing else written)
int emu_mix(const short* pcm_in, int n, int n_packets, int L, const int* room, int n_rooms, const short* gain, int max_speakers, short* pcm_out,
            long long* energy, unsigned char* mixed, void* count) {
    SxMixArgs a;
    a.pcm_in = pcm_in; a.gain = gain; a.pcm_out = pcm_out; a.energy = (i64*)energy; a.mixed = mixed;
    a.counts = 0; a.starts = 0; a.members = 0;
    a.n_packets = n_packets; a.L = L; a.max_speakers = max_speakers;
    return sx_mix_host(a, room, n, n_rooms, (SxMixCount*)count) ? 0 : -1;
}

int emu_mix_before(long long ea, int ia, long long eb, int ib) { return sx_mix_before(ea, ia, eb, ib) ? 1 : 0; }
int emu_mix_contrib(int x, int g) { return sx_mix_contrib(x, g); }

}

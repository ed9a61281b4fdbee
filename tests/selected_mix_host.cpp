// Host build of the shared mixing bridge with a given selection (solo_amd/csrc/solo_mix_selected.h) for tests/test_selected_mix_model.py,
// which compiles this file into a temporary directory through tests/host_build.py -- and, with -DSELECTED_MIX_MAIN, as a
// stand-alone program (the sanitiser build): it reads one case from a file, runs the host form and writes every output to a second file.
// The host forms of solo_mix and solo_mix_shared are exported as well: the identities of the test run against them.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../solo_amd/csrc/solo_mix_selected.h"

extern "C" {

int emu_mixsel_count_size() { return (int)sizeof(SxMixSelCount); }
long long emu_mixsel_scratch_bytes(int n, int n_packets) { return (long long)solo_mixsel_scratch_bytes(n, n_packets); }

// -> 0; -1: refused by the host checks (nothing written); -2: refused by the device checks (count->rows = -1, nothing else written)
int emu_mix_selected(const short* pcm_in, int n, int n_packets, int L, const int* room, int n_rooms, const short* gain, const unsigned char* sel,
                     const unsigned char* keep, const int* slots, short* pcm_spk, int* spk_list, int* spk_rows, short* pcm_room, int* room_list,
                     int* source, unsigned char* room_nsel, long long* energy, void* count) {
    if (!sx_mixsel_args_ok(pcm_in, n, n_packets, L, room, n_rooms, sel, pcm_spk, spk_list, pcm_room, room_list, source, count)) return -1;
    SxMixSelArgs a;
    memset(&a, 0, sizeof(a));
    a.sh.pcm_in = pcm_in; a.sh.gain = gain; a.sh.room = room; a.sh.keep = keep; a.sh.slots = slots;
    a.sh.pcm_spk = pcm_spk; a.sh.spk_list = spk_list; a.sh.spk_rows = spk_rows; a.sh.pcm_room = pcm_room; a.sh.room_list = room_list; a.sh.source = source;
    a.sh.energy = (i64*)energy; a.sh.mixed = (u8*)sel;
    a.sh.n = n; a.sh.n_rooms = n_rooms; a.sh.n_packets = n_packets; a.sh.L = L; a.sh.max_speakers = SX_MIX_MAX_SPEAKERS;
    a.room_nsel = room_nsel;
    return sx_mixsel_host(a, (SxMixSelCount*)count) ? 0 : -2;
}

// solo_mix_shared's host form, as tests/shared_mix_host.cpp exports it
int emu_mix_shared(const short* pcm_in, int n, int n_packets, int L, const int* room, int n_rooms, const short* gain, int max_speakers,
                   const unsigned char* keep, const int* slots, short* pcm_spk, int* spk_list, int* spk_rows, short* pcm_room, int* room_list,
                   int* source, long long* energy, unsigned char* mixed, void* count) {
    if (!sx_mixsh_args_ok(pcm_in, n, n_packets, L, room, n_rooms, max_speakers, pcm_spk, spk_list, pcm_room, room_list, source, count)) return -1;
    SxMixShArgs a;
    memset(&a, 0, sizeof(a));
    a.pcm_in = pcm_in; a.gain = gain; a.room = room; a.keep = keep; a.slots = slots;
    a.pcm_spk = pcm_spk; a.spk_list = spk_list; a.spk_rows = spk_rows; a.pcm_room = pcm_room; a.room_list = room_list; a.source = source;
    a.energy = (i64*)energy; a.mixed = mixed;
    a.n = n; a.n_rooms = n_rooms; a.n_packets = n_packets; a.L = L; a.max_speakers = max_speakers;
    return sx_mixsh_host(a, (SxMixShCount*)count) ? 0 : -2;
}

// solo_mix's host form, as tests/mix_host.cpp exports it
int emu_mix(const short* pcm_in, int n, int n_packets, int L, const int* room, int n_rooms, const short* gain, int max_speakers, short* pcm_out,
            long long* energy, unsigned char* mixed, void* count) {
    SxMixArgs a;
    a.pcm_in = pcm_in; a.gain = gain; a.pcm_out = pcm_out; a.energy = (i64*)energy; a.mixed = mixed;
    a.counts = 0; a.starts = 0; a.members = 0;
    a.n_packets = n_packets; a.L = L; a.max_speakers = max_speakers;
    return sx_mix_host(a, room, n, n_rooms, (SxMixCount*)count) ? 0 : -1;
}

}

#ifdef SELECTED_MIX_MAIN
// in:  int32 {n, P, L, n_rooms, with_gain, with_keep, with_slots, with_optional}, pcm int16 [n][P][L], room int32 [n], gain int16 [n],
//      sel uint8 [n][P], keep uint8 [n], slots int32 [n]
// out: int32 ret, then pcm_spk, spk_list, spk_rows, pcm_room, room_list, source, room_nsel, energy, count (32 bytes) in the sizes of the
//      interface, all of them starting from zero bytes.  Every buffer is a heap block of its exact size: an access past an end is found.
template <typename T>
static T* block(size_t count, FILE* f) {
    void* v = NULL;
    if (posix_memalign(&v, 16, count * sizeof(T))) exit(3);
    T* p = (T*)v;
    memset(p, 0, count * sizeof(T));
    if (f && fread(p, sizeof(T), count, f) != count) exit(4);
    return p;
}
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int h[8];
    if (fread(h, sizeof(int), 8, f) != 8) return 4;
    const size_t n = (size_t)h[0], P = (size_t)h[1], L = (size_t)h[2], R = (size_t)h[3];
    short* pcm = block<short>(n * P * L, f);
    int* room = block<int>(n, f);
    short* gain = block<short>(n, f);
    unsigned char* sel = block<unsigned char>(n * P, f);
    unsigned char* keep = block<unsigned char>(n, f);
    int* slots = block<int>(n, f);
    fclose(f);
    short* pcm_spk = block<short>(n * P * L, NULL);
    int* spk_list = block<int>(n, NULL);
    int* spk_rows = block<int>(n, NULL);
    short* pcm_room = block<short>(R * P * L, NULL);
    int* room_list = block<int>(R, NULL);
    int* source = block<int>(n, NULL);
    unsigned char* room_nsel = block<unsigned char>(R * P, NULL);
    long long* energy = block<long long>(n * P, NULL);
    int* count = block<int>(8, NULL);
    const int ret = emu_mix_selected(pcm, (int)n, (int)P, (int)L, room, (int)R, h[4] ? gain : NULL, sel, h[5] ? keep : NULL, h[6] ? slots : NULL, pcm_spk,
                                     spk_list, h[7] ? spk_rows : NULL, pcm_room, room_list, source, h[7] ? room_nsel : NULL, h[7] ? energy : NULL, count);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(&ret, sizeof(int), 1, o);
    fwrite(pcm_spk, sizeof(short), n * P * L, o); fwrite(spk_list, sizeof(int), n, o); fwrite(spk_rows, sizeof(int), n, o);
    fwrite(pcm_room, sizeof(short), R * P * L, o); fwrite(room_list, sizeof(int), R, o); fwrite(source, sizeof(int), n, o);
    fwrite(room_nsel, 1, R * P, o); fwrite(energy, sizeof(long long), n * P, o); fwrite(count, sizeof(int), 8, o);
    fclose(o);
    free(pcm); free(room); free(gain); free(sel); free(keep); free(slots); free(pcm_spk); free(spk_list); free(spk_rows); free(pcm_room);
    free(room_list); free(source); free(room_nsel); free(energy); free(count);
    return 0;
}
#endif

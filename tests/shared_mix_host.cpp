// Host build of the shared mixing bridge and the fan-out sender (solo_amd/csrc/solo_mix_shared.h, solo_fanout.h) for
// tests/test_shared_mix_model.py, which compiles this file into a temporary directory through tests/host_build.py.
#include <string.h>
#include "../solo_amd/csrc/solo_mix_shared.h"
#include "../solo_amd/csrc/solo_fanout.h"

extern "C" {

int emu_mixsh_count_size() { return (int)sizeof(SxMixShCount); }

// -> 0; -1: refused by the host checks (nothing written); -2: refused by the device checks (count->rows = -1, nothing else written)
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

// -> 0; -1: refused by the host checks; -2: refused by the device check (count->records = -1, nothing else written)
int emu_send_fanout(const unsigned char* bits, const short* nbytes, int n_src, const int* source, const int* dst_stream, int n_dst,
                    const unsigned char* send, int n_packets, int slot, int hbb, const int* seq_base, int first_seq, void* records, int max_records,
                    unsigned char* payload, long long cap, void* count) {
    if (!sx_fan_args_ok(bits, nbytes, n_src, source, n_dst, n_packets, records, max_records, payload, cap, count)) return -1;
    SxFanArgs a;
    memset(&a, 0, sizeof(a));
    a.bits = bits; a.nbytes = nbytes; a.source = source; a.dst_stream = dst_stream; a.send = send; a.seq_base = seq_base;
    a.n_src = n_src; a.n_dst = n_dst; a.n_packets = n_packets; a.slot = slot; a.hbb = hbb; a.first_seq = first_seq;
    return sx_fan_host(a, (SxSendRecord*)records, max_records, payload, cap, (SxSendCount*)count) ? 0 : -2;
}

}

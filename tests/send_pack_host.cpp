// Host build of the sender back end (solo_amd/csrc/solo_send.h) and of the wave scan's host form (solo_wave.h) for
// tests/test_send_pack_model.py, which compiles this file into a temporary directory through tests/host_build.py.
#include <string.h>
#include "../solo_amd/csrc/solo_send.h"

extern "C" {

int emu_send_count_size() { return (int)sizeof(SxSendCount); }

// out5 = {why, len0, len1, src1, seq}
void emu_send_plan(int total, int n1, int slot, int hbb, int mask, long long seq, int* out5) {
    const SxSendPlan p = sx_send_plan(total, n1, slot, hbb, mask, seq);
    out5[0] = p.why; out5[1] = p.len0; out5[2] = p.len1; out5[3] = p.src1; out5[4] = p.seq;
}

void emu_send_pack(const unsigned char* bits, const short* nbytes, const unsigned char* send, const int* seq_base, const int* map, int n, int n_packets,
                   int slot, int hbb, int first_seq, void* records, int max_records, unsigned char* payload, long long cap, void* count) {
    SxSendArgs a;
    a.bits = bits; a.nbytes = nbytes; a.send = send; a.seq_base = seq_base; a.map = map;
    a.n = n; a.n_packets = n_packets; a.slot = slot; a.hbb = hbb; a.first_seq = first_seq;
    sx_send_pack_host(a, (SxSendRecord*)records, max_records, payload, cap, (SxSendCount*)count);
}

void emu_send_copy(unsigned char* dst, const unsigned char* src, int n) {
    for (int lane = 0; lane < SX_SEND_ROW; lane++) sx_send_copy(dst, src, n, lane, SX_SEND_ROW);
}

void emu_wave_scan(int* v64) { wv_scan_incl_steps(v64); }

}

// Host build of the RTP stage (solo_amd/csrc/solo_rtp.h) for tests/test_rtp_model.py, which compiles this file into a temporary
// directory through tests/host_build.py.  The session is the host mirror of solo_api.hip's object: the same bind / unbind
// functions, with the "device" records and table kept in vectors.
#include <string.h>
#include "../solo_amd/csrc/solo_dec.h"
#include "../solo_amd/csrc/solo_rtp.h"

struct EmuRtp {
    SxRtpMirror m;
    std::vector<u32> table;
    int L;
};

extern "C" {

int emu_rtp_sizes(int which) {
    return which == 0 ? (int)sizeof(SxRtpDgram) : which == 1 ? (int)sizeof(SxRtpPackCount) : which == 2 ? (int)sizeof(SxRtpParseCount) : (int)sizeof(SxRtpStream);
}

void* emu_rtp_create(int n_streams, int packet_samples) {
    EmuRtp* r = new EmuRtp();
    const SxRtpStream z = {0, 0, 0, 0};
    r->m.cfg.assign((size_t)n_streams, z);
    r->m.level_id = 0;
    r->L = packet_samples;
    sx_rtp_table(r->m.cfg, 0, r->table);
    return r;
}
void emu_rtp_destroy(void* h) { delete (EmuRtp*)h; }

int emu_rtp_bind(void* h, const int* streams, int n, const unsigned* ssrc, const unsigned* ts_offset, const unsigned short* seq_offset,
                 const unsigned char* pt_md1, const unsigned char* pt_md2, int level_id) {
    EmuRtp* r = (EmuRtp*)h;
    std::vector<SxStreamCtl> recs;
    std::vector<u32> table;
    SxRtpMirror next;
    const SxRtpMirror before = r->m;
    const bool ok = sx_rtp_bind_plan(r->m, streams, n, ssrc, ts_offset, seq_offset, pt_md1, pt_md2, level_id, next, recs, table);
    // the plan never touches the mirror: the caller commits it once the device side has succeeded
    if (before.level_id != r->m.level_id || memcmp(before.cfg.data(), r->m.cfg.data(), before.cfg.size() * sizeof(SxRtpStream)) != 0) return -3;
    if (!ok) return -1;
    r->m = next;
    // what solo_rtp_bind_kernel makes of the records must be what the mirror holds
    for (int i = 0; i < n; i++) {
        const SxRtpStream& c = r->m.cfg[(size_t)recs[i].stream];
        if (c.ssrc != (u32)recs[i].a || c.ts_offset != (u32)recs[i].b || c.seq_pt != (u32)recs[i].c || c.bound != 1) return -2;
    }
    r->table.swap(table);
    return 0;
}
int emu_rtp_unbind(void* h, const int* streams, int n) {
    EmuRtp* r = (EmuRtp*)h;
    std::vector<u32> table;
    SxRtpMirror next;
    if (!sx_rtp_unbind_plan(r->m, streams, n, next, table)) return -1;
    r->m = next;
    r->table.swap(table);
    return 0;
}
// the table as the device would hold it: {bound, level id, 0, 0}, then the pairs -> words copied
int emu_rtp_table(void* h, unsigned* out, int max_words) {
    EmuRtp* r = (EmuRtp*)h;
    const int n = (int)r->table.size() < max_words ? (int)r->table.size() : max_words;
    memcpy(out, r->table.data(), (size_t)n * sizeof(u32));
    return n;
}

void emu_rtp_pack(void* h, const void* records, const void* send_count, int max_records, const unsigned char* payload, long long payload_bytes,
                  const unsigned char* level, int level_depth, void* dgrams, unsigned char* wire, long long cap, void* count) {
    EmuRtp* r = (EmuRtp*)h;
    SxRtpPackArgs a;
    a.records = (const SxSendRecord*)records; a.send_count = (const SxSendCount*)send_count; a.payload = payload; a.level = level;
    a.cfg = r->m.cfg.data(); a.table = r->table.data(); a.payload_bytes = payload_bytes;
    a.max_records = max_records; a.n_streams = (int)r->m.cfg.size(); a.level_depth = level_depth; a.packet_samples = r->L;
    sx_rtp_pack_host(a, (SxRtpDgram*)dgrams, wire, cap, (SxRtpPackCount*)count);
}

void emu_rtp_parse(void* h, const int* play, const void* dgrams, int n_dgrams, const unsigned char* wire, long long wire_bytes, void* arrivals,
                   unsigned char* level_out, unsigned short* rtp_seq_out, void* count) {
    EmuRtp* r = (EmuRtp*)h;
    SxRtpParseArgs a;
    a.dgrams = (const SxRtpDgram*)dgrams; a.wire = wire; a.cfg = r->m.cfg.data(); a.table = r->table.data(); a.play = play;
    a.wire_bytes = wire_bytes > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : wire_bytes;
    a.n_dgrams = n_dgrams; a.n_streams = (int)r->m.cfg.size(); a.packet_samples = r->L;
    sx_rtp_parse_host(a, (SxSendRecord*)arrivals, level_out, rtp_seq_out, (SxRtpParseCount*)count);
}

}

// Host build of the SRTP stage (solo_amd/csrc/solo_srtp.h, with the pack of solo_rtp.h in front of it) for tests/test_srtp_model.py, which
// compiles this file through tests/host_build.py.  The session is the host mirror of solo_api.hip's object: the same plan functions, with
// the "device" records kept in vectors.  With -DSRTP_MAIN the same source is a stand-alone program (the sanitiser run of the test): one
// unprotect call in through a file, every output back through a file.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../solo_amd/csrc/solo_dec.h"
#include "../solo_amd/csrc/solo_srtp.h"

struct EmuSrtp {
    SxRtpMirror m;
    std::vector<u32> table;
    int L, trailer;
    bool allocated;
    std::vector<SxSrtpKey> keys;     // [n_streams][2]
    std::vector<SxSrtpRx> rx;
    SxSrtpMirror srtp;
};

static void emu_clear(EmuSrtp* r, const int* streams, int n) {
    if (!r->allocated) return;
    for (int i = 0; i < n; i++) {
        memset(&r->keys[2 * (size_t)streams[i]], 0, 2 * sizeof(SxSrtpKey));
        SxSrtpRx x; memset(&x, 0, sizeof(x)); x.index = -1;
        r->rx[(size_t)streams[i]] = x;
        r->srtp.tx_tag[(size_t)streams[i]] = 0; r->srtp.rx_tag[(size_t)streams[i]] = 0;
    }
}

extern "C" {

int emu_srtp_sizes(int which) { return which == 0 ? (int)sizeof(SxSrtpCount) : which == 1 ? (int)sizeof(SxSrtpKey) : which == 2 ? (int)sizeof(SxSrtpRx) : (int)sizeof(SxSrtpRun); }

// ---- the pieces, for the published answers ------------------------------------------------------------------------------------------------
void emu_aes_block(const unsigned char* key, const unsigned char* in, unsigned char* out) {
    u32 rk[44], s[4], o[4];
    sx_aes_expand(key, rk);
    for (int k = 0; k < 4; k++) s[k] = ((u32)in[4 * k] << 24) | ((u32)in[4 * k + 1] << 16) | ((u32)in[4 * k + 2] << 8) | in[4 * k + 3];
    sx_aes_block(rk, SX_AES_TE0, s[0], s[1], s[2], s[3], o);
    for (int k = 0; k < 16; k++) out[k] = (unsigned char)(o[k >> 2] >> (8 * (3 - (k & 3))));
}
void emu_aes_cm(const unsigned char* key, const unsigned char* iv16, unsigned j, unsigned char* out) {
    u32 rk[44], iv[4], o[4];
    sx_aes_expand(key, rk);
    for (int k = 0; k < 4; k++) iv[k] = ((u32)iv16[4 * k] << 24) | ((u32)iv16[4 * k + 1] << 16) | ((u32)iv16[4 * k + 2] << 8) | iv16[4 * k + 3];
    sx_aes_cm_block(rk, SX_AES_TE0, iv, j, o);
    for (int k = 0; k < 16; k++) out[k] = (unsigned char)(o[k >> 2] >> (8 * (3 - (k & 3))));
}
void emu_srtp_derive(const unsigned char* master30, unsigned char* ke16, unsigned char* ks14, unsigned char* ka20, unsigned* record64) {
    SxSrtpKey rec;
    sx_srtp_make_key(master30, 10, &rec, ke16, ks14, ka20);
    memcpy(record64, &rec, sizeof(rec));
}
// HMAC-SHA1 the way the kernels compute it: from the two midstates, the message at any alignment, n_roc = 0 (the bare message) or 4
void emu_hmac(const unsigned char* key, int key_bytes, const unsigned char* msg, int n, unsigned roc, int n_roc, unsigned char* out20) {
    u32 mi[5], mo[5], tag[5];
    sx_hmac_midstates(key, key_bytes, mi, mo);
    sx_srtp_mac(mi, mo, msg, n, roc, n_roc, tag);
    for (int k = 0; k < 20; k++) out20[k] = (unsigned char)(tag[k >> 2] >> (8 * (3 - (k & 3))));
}
long long emu_srtp_guess(long long index, unsigned roc0, unsigned seq) {
    SxSrtpRx x; memset(&x, 0, sizeof(x)); x.index = index; x.roc0 = roc0;
    return sx_srtp_guess_index(x, seq);
}

// ---- the session ------------------------------------------------------------------------------------------------------------------------------
void* emu_srtp_create(int n_streams, int packet_samples) {
    EmuSrtp* r = new EmuSrtp();
    const SxRtpStream z = {0, 0, 0, 0};
    r->m.cfg.assign((size_t)n_streams, z);
    r->m.level_id = 0;
    r->L = packet_samples; r->trailer = 0; r->allocated = false;
    sx_rtp_table(r->m.cfg, 0, r->table);
    return r;
}
void emu_srtp_destroy(void* h) { delete (EmuSrtp*)h; }
int emu_srtp_bind(void* h, const int* streams, int n, const unsigned* ssrc, const unsigned* ts_offset, const unsigned short* seq_offset,
                  const unsigned char* pt_md1, const unsigned char* pt_md2, int level_id) {
    EmuSrtp* r = (EmuSrtp*)h;
    std::vector<SxStreamCtl> recs;
    std::vector<u32> table;
    SxRtpMirror next;
    if (!sx_rtp_bind_plan(r->m, streams, n, ssrc, ts_offset, seq_offset, pt_md1, pt_md2, level_id, next, recs, table)) return -1;
    r->m = next;
    r->table.swap(table);
    return 0;
}
int emu_srtp_unbind(void* h, const int* streams, int n) {
    EmuSrtp* r = (EmuSrtp*)h;
    std::vector<u32> table;
    SxRtpMirror next;
    if (!sx_rtp_unbind_plan(r->m, streams, n, next, table)) return -1;
    emu_clear(r, streams, n);
    r->m = next;
    r->table.swap(table);
    return 0;
}
int emu_srtp_set_trailer(void* h, int trailer) {
    EmuSrtp* r = (EmuSrtp*)h;
    if (!sx_srtp_trailer_ok(r->srtp, trailer)) return -1;
    r->trailer = trailer;
    return 0;
}
int emu_srtp_set_keys(void* h, const int* streams, int n, const unsigned char* tx, const unsigned char* rx, const unsigned* roc, int tag_bytes) {
    EmuSrtp* r = (EmuSrtp*)h;
    std::vector<SxSrtpKey> recs;
    std::vector<SxSrtpRx> rxs;
    SxSrtpMirror next;
    const int N = (int)r->m.cfg.size();
    if (!sx_srtp_set_keys_plan(r->srtp, N, r->trailer, streams, n, tx, rx, roc, tag_bytes, next, recs, rxs)) return -1;
    if (!r->allocated) {
        SxSrtpKey zk; memset(&zk, 0, sizeof(zk));
        SxSrtpRx zx; memset(&zx, 0, sizeof(zx)); zx.index = -1;
        r->keys.assign(2 * (size_t)N, zk); r->rx.assign((size_t)N, zx);
        r->allocated = true;
    }
    for (int i = 0; i < n; i++) {
        if (tx) r->keys[2 * (size_t)streams[i]] = recs[2 * (size_t)i];
        if (rx) { r->keys[2 * (size_t)streams[i] + 1] = recs[2 * (size_t)i + 1]; r->rx[(size_t)streams[i]] = rxs[(size_t)i]; }
    }
    sx_srtp_wipe(recs);
    r->srtp = next;
    return 0;
}
int emu_srtp_clear_keys(void* h, const int* streams, int n) {
    EmuSrtp* r = (EmuSrtp*)h;
    if (!sx_list_ok(streams, n, (int)r->m.cfg.size())) return -1;
    emu_clear(r, streams, n);
    return 0;
}
int emu_srtp_rx_index(void* h, const int* streams, int n, long long* index) {
    EmuSrtp* r = (EmuSrtp*)h;
    if (!index || !sx_list_ok(streams, n, (int)r->m.cfg.size())) return -1;
    for (int i = 0; i < n; i++) index[i] = r->allocated ? (long long)r->rx[(size_t)streams[i]].index : -1;
    return 0;
}
// the mirror: tag of the tx (which = 0) or rx key of a stream, 0 = none
int emu_srtp_mirror(void* h, int stream, int which) {
    EmuSrtp* r = (EmuSrtp*)h;
    if (!r->allocated) return 0;
    return which ? r->srtp.rx_tag[(size_t)stream] : r->srtp.tx_tag[(size_t)stream];
}
// words of the key records that are not zero, over the whole session (what a clear must leave at 0 for its streams)
int emu_srtp_key_words(void* h, int stream) {
    EmuSrtp* r = (EmuSrtp*)h;
    if (!r->allocated) return 0;
    int n = 0;
    const u32* w = (const u32*)&r->keys[2 * (size_t)stream];
    for (int k = 0; k < 2 * SOLO_SRTP_KEY_WORDS; k++) n += w[k] != 0;
    return n;
}

void emu_srtp_pack(void* h, const void* records, const void* send_count, int max_records, const unsigned char* payload, long long payload_bytes,
                   const unsigned char* level, int level_depth, void* dgrams, unsigned char* wire, long long cap, void* count) {
    EmuSrtp* r = (EmuSrtp*)h;
    SxRtpPackArgs a;
    a.records = (const SxSendRecord*)records; a.send_count = (const SxSendCount*)send_count; a.payload = payload; a.level = level;
    a.cfg = r->m.cfg.data(); a.table = r->table.data(); a.payload_bytes = payload_bytes;
    a.max_records = max_records; a.n_streams = (int)r->m.cfg.size(); a.level_depth = level_depth; a.packet_samples = r->L; a.trailer = r->trailer;
    sx_rtp_pack_host(a, (SxRtpDgram*)dgrams, wire, cap, (SxRtpPackCount*)count);
}
void emu_srtp_protect(void* h, const void* records, const void* send_count, int max_records, void* dgrams, unsigned char* wire, long long wire_bytes, void* count) {
    EmuSrtp* r = (EmuSrtp*)h;
    SxSrtpProtectArgs a;
    a.records = (const SxSendRecord*)records; a.send_count = (const SxSendCount*)send_count; a.dgrams = (SxRtpDgram*)dgrams; a.wire = wire;
    a.cfg = r->m.cfg.data(); a.keys = r->allocated ? r->keys.data() : NULL;
    a.wire_bytes = wire_bytes > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : wire_bytes;
    a.max_records = max_records; a.n_streams = (int)r->m.cfg.size();
    sx_srtp_protect_host(a, (SxSrtpCount*)count);
}
void emu_srtp_unprotect(void* h, const void* dgrams, int n_dgrams, unsigned char* wire, long long wire_bytes, void* dgrams_out, void* count) {
    EmuSrtp* r = (EmuSrtp*)h;
    SxSrtpUnprotectArgs a;
    a.dgrams = (const SxRtpDgram*)dgrams; a.out = (SxRtpDgram*)dgrams_out; a.wire = wire; a.table = r->table.data();
    a.keys = r->allocated ? r->keys.data() : NULL; a.rx = r->allocated ? r->rx.data() : NULL;
    a.wire_bytes = wire_bytes > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : wire_bytes;
    a.n_dgrams = n_dgrams; a.n_streams = (int)r->m.cfg.size();
    sx_srtp_unprotect_host(a, (SxSrtpCount*)count);
}

}

#if defined(SRTP_MAIN)
// in:  int32 {n_streams, n_dgrams, wire_bytes, tag, 0, 0, 0, 0}; uint32 ssrc [n_streams]; uint32 roc [n_streams]; uint8 rx master
//      [n_streams][30]; int32 dgrams [n_dgrams][2]; uint8 wire [wire_bytes]
// out: int32 dgrams_out [n_dgrams][2]; int32 count [8]; int64 rx index [n_streams]; uint8 wire [wire_bytes]
// Every buffer is a heap block of exactly its size, so a read or write one byte outside it is a report.
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[8];
    if (fread(hdr, 4, 8, f) != 8) return 2;
    const int N = hdr[0], n = hdr[1], wb = hdr[2], tag = hdr[3];
    unsigned* ssrc = (unsigned*)malloc(4 * (size_t)N);
    unsigned* roc = (unsigned*)malloc(4 * (size_t)N);
    unsigned char* master = (unsigned char*)malloc(30 * (size_t)N);
    int* dg = (int*)malloc(8 * (size_t)n);
    unsigned char* wire = (unsigned char*)malloc((size_t)wb);
    if (fread(ssrc, 4, (size_t)N, f) != (size_t)N || fread(roc, 4, (size_t)N, f) != (size_t)N || fread(master, 30, (size_t)N, f) != (size_t)N ||
        fread(dg, 8, (size_t)n, f) != (size_t)n || fread(wire, 1, (size_t)wb, f) != (size_t)wb)
        return 2;
    fclose(f);
    void* h = emu_srtp_create(N, 640);
    int* streams = (int*)malloc(4 * (size_t)N);
    unsigned* zero = (unsigned*)calloc((size_t)N, 4);
    unsigned short* seq0 = (unsigned short*)calloc((size_t)N, 2);
    unsigned char* pt = (unsigned char*)malloc((size_t)N);
    for (int s = 0; s < N; s++) { streams[s] = s; pt[s] = 96; }
    if (emu_srtp_bind(h, streams, N, ssrc, zero, seq0, pt, pt, 0) != 0) return 3;
    if (emu_srtp_set_keys(h, streams, N, NULL, master, roc, tag) != 0) return 3;
    int* out = (int*)malloc(8 * (size_t)n);
    int count[8];
    long long* index = (long long*)malloc(8 * (size_t)N);
    emu_srtp_unprotect(h, dg, n, wire, wb, out, count);
    emu_srtp_rx_index(h, streams, N, index);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out, 8, (size_t)n, f); fwrite(count, 4, 8, f); fwrite(index, 8, (size_t)N, f); fwrite(wire, 1, (size_t)wb, f);
    fclose(f);
    emu_srtp_destroy(h);
    free(ssrc); free(roc); free(master); free(dg); free(wire); free(streams); free(zero); free(seq0); free(pt); free(out); free(index);
    return 0;
}
#endif

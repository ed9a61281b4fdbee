// Host build of AEAD_AES_128_GCM in the SRTP and the SRTCP stage (solo_amd/csrc/solo_srtp_gcm.h) for tests/test_srtp_gcm_model.py, which
// compiles this file through tests/host_build.py.  The two sessions are those of tests/srtp_host.cpp and tests/srtcp_host.cpp, taken in as
// they are (their emu_srtp_* / emu_srtcp_* / emu_rtcp_* calls are exported from this library too); the calls added here set GCM keys
// beside theirs and run the four device calls the way solo_api.hip issues them: the older transform's pass, this one's behind it, the fold
// last.  With -DSRTP_GCM_MAIN the same source is a stand-alone program (the sanitiser run of the test): one unprotect call of either stage
// in through a file, every output back through a file.
#include "srtp_host.cpp"
#include "srtcp_host.cpp"
#include "../solo_amd/csrc/solo_srtp_gcm.h"

static void gcm_words(const unsigned char* b, int n_words, u32* w) {
    for (int k = 0; k < n_words; k++) w[k] = ((u32)b[4 * k] << 24) | ((u32)b[4 * k + 1] << 16) | ((u32)b[4 * k + 2] << 8) | b[4 * k + 3];
}
static void gcm_bytes(const u32* w, int n_words, unsigned char* b) {
    for (int k = 0; k < 4 * n_words; k++) b[k] = (unsigned char)(w[k >> 2] >> (8 * (3 - (k & 3))));
}

extern "C" {

int emu_gcm_sizes(int which) { return which == 0 ? SX_GCM_TAG : which == 1 ? SX_SRTCP_GCM_TRAILER : which == 2 ? SX_GCM_MASTER : which == 3 ? SX_GCM_TILE : (int)sizeof(SxSrtpKey); }

// ---- the pieces -------------------------------------------------------------------------------------------------------------------------------
// out = x . h through the table, with the table laid out at `stride` words (1, or a tile's)
void emu_gcm_mul(const unsigned char* h16, const unsigned char* x16, int stride, unsigned char* out16) {
    u32 h[4], y[4];
    std::vector<u32> tab((size_t)SX_GCM_TABLE_WORDS * (size_t)stride, 0xDEADBEEFu);
    gcm_words(h16, 4, h); gcm_words(x16, 4, y);
    sx_gcm_table(h, tab.data() + (stride - 1), stride);
    sx_gcm_mul(y, tab.data() + (stride - 1), stride, SX_GCM_RED);
    gcm_bytes(y, 4, out16);
}
void emu_gcm_ghash(const unsigned char* h16, const unsigned char* aad, int n_aad, unsigned word, int n_word, const unsigned char* ct, int n_ct, unsigned char* out16) {
    u32 h[4], y[4], tab[SX_GCM_TABLE_WORDS];
    gcm_words(h16, 4, h);
    sx_gcm_table(h, tab, 1);
    sx_gcm_ghash(tab, 1, SX_GCM_RED, aad, n_aad, word, n_word, ct, n_ct, y);
    gcm_bytes(y, 4, out16);
}
// AES-128-GCM with a 12-byte IV over buf[0 .. n) in place, by the record, cipher and tag functions the kernels run -> the tag
void emu_gcm_encrypt(const unsigned char* key16, const unsigned char* iv12, const unsigned char* aad, int n_aad, unsigned char* buf, int n, unsigned char* tag16) {
    SxSrtpKey rec;
    sx_srtp_gcm_session_record(key16, iv12, &rec);          // (the salt's place holds the IV: SSRC, ROC and SEQ are 0 below)
    u32 iv[3], tag[4], tab[SX_GCM_TABLE_WORDS];
    for (int lane = 0; lane < SX_RTP_ROW; lane++) sx_gcm_cipher(buf, 0, n, &rec, SX_AES_TE0, 0, 0, 0, lane, SX_RTP_ROW);
    sx_gcm_table(rec.mid_i, tab, 1);
    sx_gcm_iv(&rec, 0, 0, 0, iv);
    sx_gcm_tag(&rec, SX_AES_TE0, iv, tab, 1, SX_GCM_RED, aad, n_aad, 0u, 0, buf, n, tag);
    gcm_bytes(tag, 4, tag16);
}
void emu_gcm_derive(const unsigned char* master28, int label, unsigned char* ke16, unsigned char* ks12, unsigned* record64) {
    SxSrtpKey rec;
    sx_srtp_gcm_make_key_at(master28, label, &rec, ke16, ks12);
    memcpy(record64, &rec, sizeof(rec));
}

// ---- SRTP: the session of tests/srtp_host.cpp ----------------------------------------------------------------------------------------------------
static void gcm_srtp_alloc(EmuSrtp* r) {
    if (r->allocated) return;
    const size_t N = r->m.cfg.size();
    SxSrtpKey zk; memset(&zk, 0, sizeof(zk));
    SxSrtpRx zx; memset(&zx, 0, sizeof(zx)); zx.index = -1;
    r->keys.assign(2 * N, zk); r->rx.assign(N, zx);
    r->srtp.tx_tag.assign(N, 0); r->srtp.rx_tag.assign(N, 0);
    r->allocated = true;
}
int emu_gcm_srtp_set_keys(void* h, const int* streams, int n, const unsigned char* tx, const unsigned char* rx, const unsigned* roc) {
    EmuSrtp* r = (EmuSrtp*)h;
    std::vector<SxSrtpKey> recs;
    std::vector<SxSrtpRx> rxs;
    SxSrtpMirror next;
    if (!sx_srtp_gcm_set_keys_plan(r->srtp, (int)r->m.cfg.size(), r->trailer, streams, n, tx, rx, roc, next, recs, rxs)) return -1;
    gcm_srtp_alloc(r);
    for (int i = 0; i < n; i++) {
        if (tx) r->keys[2 * (size_t)streams[i]] = recs[2 * (size_t)i];
        if (rx) { r->keys[2 * (size_t)streams[i] + 1] = recs[2 * (size_t)i + 1]; r->rx[(size_t)streams[i]] = rxs[(size_t)i]; }
    }
    sx_srtp_wipe(recs);
    r->srtp = next;
    return 0;
}
// test only: a direction's record from SESSION key and salt (the published vectors and the fixture's datagrams give those, not masters)
int emu_gcm_srtp_set_session(void* h, int stream, int dir, const unsigned char* ke16, const unsigned char* ks12, unsigned roc) {
    EmuSrtp* r = (EmuSrtp*)h;
    if (stream < 0 || stream >= (int)r->m.cfg.size() || (dir == 0 && r->trailer < SX_GCM_TAG)) return -1;
    gcm_srtp_alloc(r);
    sx_srtp_gcm_session_record(ke16, ks12, &r->keys[2 * (size_t)stream + (dir ? 1 : 0)]);
    if (dir) {
        SxSrtpRx x; memset(&x, 0, sizeof(x)); x.index = -1; x.roc0 = roc;
        r->rx[(size_t)stream] = x;
        r->srtp.rx_tag[(size_t)stream] = SX_GCM_TAG;
    } else r->srtp.tx_tag[(size_t)stream] = SX_GCM_TAG;
    return 0;
}
void emu_gcm_srtp_record(void* h, int stream, int dir, unsigned* record64) {
    EmuSrtp* r = (EmuSrtp*)h;
    memcpy(record64, &r->keys[2 * (size_t)stream + (dir ? 1 : 0)], sizeof(SxSrtpKey));
}
// does the call enqueue this transform's kernel?  (what solo_api.hip asks of the mirror)
int emu_gcm_srtp_any(void* h, int dir) {
    EmuSrtp* r = (EmuSrtp*)h;
    return r->allocated && sx_srtp_gcm_count(dir ? r->srtp.rx_tag : r->srtp.tx_tag) > 0 ? 1 : 0;
}
void emu_gcm_srtp_protect(void* h, const void* records, const void* send_count, int max_records, void* dgrams, unsigned char* wire, long long wire_bytes, void* count) {
    EmuSrtp* r = (EmuSrtp*)h;
    SxSrtpProtectArgs a;
    a.records = (const SxSendRecord*)records; a.send_count = (const SxSendCount*)send_count; a.dgrams = (SxRtpDgram*)dgrams; a.wire = wire;
    a.cfg = r->m.cfg.data(); a.keys = r->allocated ? r->keys.data() : NULL;
    a.wire_bytes = wire_bytes > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : wire_bytes;
    a.max_records = max_records; a.n_streams = (int)r->m.cfg.size();
    if (emu_gcm_srtp_any(h, 0)) sx_srtp_protect_host_all(a, (SxSrtpCount*)count);
    else sx_srtp_protect_host(a, (SxSrtpCount*)count);
}
void emu_gcm_srtp_unprotect(void* h, const void* dgrams, int n_dgrams, unsigned char* wire, long long wire_bytes, void* dgrams_out, void* count) {
    EmuSrtp* r = (EmuSrtp*)h;
    SxSrtpUnprotectArgs a;
    a.dgrams = (const SxRtpDgram*)dgrams; a.out = (SxRtpDgram*)dgrams_out; a.wire = wire; a.table = r->table.data();
    a.keys = r->allocated ? r->keys.data() : NULL; a.rx = r->allocated ? r->rx.data() : NULL;
    a.wire_bytes = wire_bytes > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : wire_bytes;
    a.n_dgrams = n_dgrams; a.n_streams = (int)r->m.cfg.size();
    if (emu_gcm_srtp_any(h, 1)) sx_srtp_unprotect_host_all(a, (SxSrtpCount*)count);
    else sx_srtp_unprotect_host(a, (SxSrtpCount*)count);
}

// ---- SRTCP: the session of tests/srtcp_host.cpp ---------------------------------------------------------------------------------------------------
static void gcm_srtcp_alloc(EmuSrtcp* r) {
    if (!r->mem.empty()) return;
    r->mem.resize(sx_srtcp_bytes(r->n));
    sx_srtcp_mem_init(r->mem.data(), r->n);
    r->mirror.has_tx.assign((size_t)r->n, 0); r->mirror.has_rx.assign((size_t)r->n, 0);
}
int emu_gcm_srtcp_set_keys(void* h, const int* streams, int n, const unsigned char* tx, const unsigned char* rx, const unsigned* tx_index, const long long* rx_index) {
    EmuSrtcp* r = (EmuSrtcp*)h;
    std::vector<SxSrtpKey> recs;
    std::vector<SxSrtcpTx> txs;
    std::vector<SxSrtcpRx> rxs;
    SxSrtcpMirror next;
    if (!r || !sx_srtcp_gcm_set_keys_plan(r->mirror, r->n, streams, n, tx, rx, tx_index, (const i64*)rx_index, next, recs, txs, rxs)) return -1;
    gcm_srtcp_alloc(r);
    const SxSrtcpMem m = emu_mem(r);
    for (int i = 0; i < n; i++) {
        const size_t s = (size_t)streams[i];
        if (tx) { m.keys[2 * s] = recs[2 * (size_t)i]; m.tx[s] = txs[(size_t)i]; }
        if (rx) { m.keys[2 * s + 1] = recs[2 * (size_t)i + 1]; m.rx[s] = rxs[(size_t)i]; }
    }
    sx_srtp_wipe(recs);
    r->mirror = next;
    return 0;
}
// test only: a direction's record from SESSION key and salt, with its index (tx: the next to send; rx: the highest authenticated)
int emu_gcm_srtcp_set_session(void* h, int stream, int dir, const unsigned char* ke16, const unsigned char* ks12, long long index) {
    EmuSrtcp* r = (EmuSrtcp*)h;
    if (stream < 0 || stream >= r->n) return -1;
    gcm_srtcp_alloc(r);
    const SxSrtcpMem m = emu_mem(r);
    sx_srtp_gcm_session_record(ke16, ks12, &m.keys[2 * (size_t)stream + (dir ? 1 : 0)]);
    if (dir) { m.rx[stream].index = index; m.rx[stream].pending = 0; r->mirror.has_rx[(size_t)stream] = SX_SRTCP_HAS_GCM; }
    else { m.tx[stream].next = (u32)index; r->mirror.has_tx[(size_t)stream] = SX_SRTCP_HAS_GCM; }
    return 0;
}
void emu_gcm_srtcp_record(void* h, int stream, int dir, unsigned* record64) {
    EmuSrtcp* r = (EmuSrtcp*)h;
    memcpy(record64, emu_mem(r).keys + 2 * (size_t)stream + (dir ? 1 : 0), sizeof(SxSrtpKey));
}
int emu_gcm_srtcp_mirror(void* h, int stream, int dir) {
    EmuSrtcp* r = (EmuSrtcp*)h;
    if (r->mem.empty()) return 0;
    return dir ? r->mirror.has_rx[(size_t)stream] : r->mirror.has_tx[(size_t)stream];
}
// rtcp_streams / trailer: what the call reads of the RTCP object.  -> -1: refused by the argument rules, the longer trailer's among them
int emu_gcm_srtcp_protect(void* h, int rtcp_streams, int trailer, const int* streams, int n, const void* build_count, void* dgrams, unsigned char* wire,
                          long long wire_bytes, void* count) {
    EmuSrtcp* r = (EmuSrtcp*)h;
    if (!sx_srtcp_protect_ok(rtcp_streams > 0 ? (const void*)r : NULL, rtcp_streams, trailer, r, r ? r->n : 0, streams, n, build_count, dgrams, wire, wire_bytes, count) ||
        !sx_srtcp_gcm_protect_ok(sx_srtcp_gcm_count(r->mirror.has_tx) > 0, trailer))
        return -1;
    const SxSrtcpMem m = emu_mem(r);
    SxSrtcpProtectArgs a;
    a.streams = streams; a.build_count = (const SxRtcpBuildCount*)build_count; a.dgrams = (SxRtpDgram*)dgrams; a.wire = wire; a.keys = m.keys; a.tx = m.tx;
    a.wire_bytes = wire_bytes > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : wire_bytes;
    a.n = n; a.n_streams = r->n;
    if (sx_srtcp_gcm_count(r->mirror.has_tx) > 0) sx_srtcp_protect_host_all(a, (SxSrtcpCount*)count);
    else sx_srtcp_protect_host(a, (SxSrtcpCount*)count);
    return 0;
}
int emu_gcm_srtcp_unprotect(void* h, const void* dgrams, int n_dgrams, unsigned char* wire, long long wire_bytes, void* dgrams_out, void* count) {
    EmuSrtcp* r = (EmuSrtcp*)h;
    if (!sx_srtcp_unprotect_ok(r, dgrams, n_dgrams, wire, wire_bytes, dgrams_out, count)) return -1;
    const SxSrtcpMem m = emu_mem(r);
    SxSrtcpUnprotectArgs a;
    a.dgrams = (const SxRtpDgram*)dgrams; a.out = (SxRtpDgram*)dgrams_out; a.wire = wire; a.table = r->table.data(); a.keys = m.keys; a.rx = m.rx;
    a.wire_bytes = wire_bytes > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : wire_bytes;
    a.n_dgrams = n_dgrams; a.n_streams = r->n;
    if (sx_srtcp_gcm_count(r->mirror.has_rx) > 0) sx_srtcp_unprotect_host_all(a, (SxSrtcpCount*)count);
    else sx_srtcp_unprotect_host(a, (SxSrtcpCount*)count);
    return 0;
}

}

#if defined(SRTP_GCM_MAIN)
// in:  int32 {n_streams, n_dgrams, wire_bytes, stage (0 SRTP, 1 SRTCP), 0, 0, 0, 0}; uint32 ssrc [n_streams]; int64 start [n_streams] (SRTP:
//      the initial rollover counter; SRTCP: the receive index); uint8 rx master [n_streams][28]; int32 dgrams [n_dgrams][2]; uint8 wire
//      [wire_bytes]
// out: int32 dgrams_out [n_dgrams][2]; int32 count [8]; int64 rx index [n_streams]; uint8 wire [wire_bytes]
// Every buffer is a heap block of exactly its size, so a read or write one byte outside it is a report.
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[8];
    if (fread(hdr, 4, 8, f) != 8) return 2;
    const int N = hdr[0], n = hdr[1], wb = hdr[2], stage = hdr[3];
    unsigned* ssrc = (unsigned*)malloc(4 * (size_t)N);
    long long* start = (long long*)malloc(8 * (size_t)N);
    unsigned char* master = (unsigned char*)malloc(28 * (size_t)N);
    int* dg = (int*)malloc(8 * (size_t)n);
    unsigned char* wire = (unsigned char*)malloc((size_t)wb);
    if (fread(ssrc, 4, (size_t)N, f) != (size_t)N || fread(start, 8, (size_t)N, f) != (size_t)N || fread(master, 28, (size_t)N, f) != (size_t)N ||
        fread(dg, 8, (size_t)n, f) != (size_t)n || fread(wire, 1, (size_t)wb, f) != (size_t)wb)
        return 2;
    fclose(f);
    int* streams = (int*)malloc(4 * (size_t)N);
    for (int s = 0; s < N; s++) streams[s] = s;
    int* out = (int*)malloc(8 * (size_t)n);
    int count[8];
    long long* index = (long long*)malloc(8 * (size_t)N);
    if (stage == 0) {
        void* h = emu_srtp_create(N, 640);
        unsigned* zero = (unsigned*)calloc((size_t)N, 4);
        unsigned* roc = (unsigned*)malloc(4 * (size_t)N);
        unsigned short* seq0 = (unsigned short*)calloc((size_t)N, 2);
        unsigned char* pt = (unsigned char*)malloc((size_t)N);
        for (int s = 0; s < N; s++) { pt[s] = 96; roc[s] = (unsigned)start[s]; }
        if (emu_srtp_bind(h, streams, N, ssrc, zero, seq0, pt, pt, 0) != 0) return 3;
        if (emu_gcm_srtp_set_keys(h, streams, N, NULL, master, roc) != 0) return 3;
        emu_gcm_srtp_unprotect(h, dg, n, wire, wb, out, count);
        emu_srtp_rx_index(h, streams, N, index);
        emu_srtp_destroy(h);
        free(zero); free(roc); free(seq0); free(pt);
    } else {
        unsigned* cfg = (unsigned*)calloc(4 * (size_t)N, 4);
        for (int s = 0; s < N; s++) { cfg[4 * s] = ssrc[s]; cfg[4 * s + 3] = 1; }
        void* h = emu_srtcp_create(cfg, N);
        if (!h || emu_gcm_srtcp_set_keys(h, streams, N, NULL, master, NULL, start) != 0) return 3;
        if (emu_gcm_srtcp_unprotect(h, dg, n, wire, wb, out, count) != 0) return 3;
        emu_srtcp_get_index(h, streams, N, NULL, index);
        emu_srtcp_destroy(h);
        free(cfg);
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out, 8, (size_t)n, f); fwrite(count, 4, 8, f); fwrite(index, 8, (size_t)N, f); fwrite(wire, 1, (size_t)wb, f);
    fclose(f);
    free(ssrc); free(start); free(master); free(dg); free(wire); free(streams); free(out); free(index);
    return 0;
}
#endif

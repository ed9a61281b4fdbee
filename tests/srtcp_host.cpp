// Host build of the SRTCP stage (solo_amd/csrc/solo_srtcp.h) for tests/test_srtcp_model.py, which compiles this file through
// tests/host_build.py.  The RTCP object around it is that of tests/rtcp_host.cpp, taken in as it is (its emu_rtcp_* calls are exported from
// this library too); emu_srtcp_build is its build call with the trailer switch.  The session is the host mirror of what solo_api.hip keeps
// for SRTCP: the records of an RTP session, its table, and the one allocation of keys, send and receive records behind the same plan
// functions.  With -DSRTCP_MAIN the same source is a stand-alone program (the sanitiser run of the test): one unprotect call in through a
// file, every output back through a file.
#include <stdio.h>
#include <stdlib.h>
#include "rtcp_host.cpp"
#include "../solo_amd/csrc/solo_srtcp.h"

struct EmuSrtcp {
    int n;
    std::vector<SxRtpStream> cfg;
    std::vector<u32> table;
    std::vector<u8> mem;             // the allocation (SxSrtcpMem), empty until the first set_keys
    SxSrtcpMirror mirror;
};
static SxSrtcpMem emu_mem(EmuSrtcp* r) { return sx_srtcp_mem(r->mem.empty() ? NULL : r->mem.data(), r->n); }
static void emu_clear(EmuSrtcp* r, const int* streams, int n) {
    if (r->mem.empty()) return;
    const SxSrtcpMem m = emu_mem(r);
    for (int i = 0; i < n; i++) {
        memset(m.keys + 2 * (size_t)streams[i], 0, 2 * sizeof(SxSrtpKey));
        m.tx[streams[i]].next = 0; m.rx[streams[i]].index = -1; m.rx[streams[i]].pending = 0;
        r->mirror.has_tx[(size_t)streams[i]] = 0; r->mirror.has_rx[(size_t)streams[i]] = 0;
    }
}

extern "C" {

int emu_srtcp_sizes(int which) {
    return which == 0 ? (int)sizeof(SxSrtcpCount) : which == 1 ? (int)sizeof(SxSrtpKey) : which == 2 ? (int)sizeof(SxSrtcpRx) : which == 3 ? (int)sizeof(SxSrtcpTx)
         : which == 4 ? SX_SRTCP_TRAILER : (int)sx_srtcp_bytes(1);
}
void emu_srtcp_derive(const unsigned char* master30, unsigned char* ke16, unsigned char* ks14, unsigned char* ka20, unsigned* record64) {
    SxSrtpKey rec;
    sx_srtp_make_key_at(master30, 3, SX_SRTCP_TAG, &rec, ke16, ks14, ka20);
    memcpy(record64, &rec, sizeof(rec));
}

// ---- the session: cfg uint32 [n][4] as rtcp_model.Session.cfg() gives it ---------------------------------------------------------------------
void* emu_srtcp_create(const unsigned* cfg, int n) {
    EmuSrtcp* r = new EmuSrtcp();
    r->n = n;
    r->cfg.resize((size_t)n);
    memcpy(r->cfg.data(), cfg, (size_t)n * sizeof(SxRtpStream));
    if (!sx_rtp_table(r->cfg, 0, r->table)) { delete r; return NULL; }
    return r;
}
void emu_srtcp_destroy(void* h) { delete (EmuSrtcp*)h; }
int emu_srtcp_unbind(void* h, const int* streams, int n) {
    EmuSrtcp* r = (EmuSrtcp*)h;
    if (!sx_list_ok(streams, n, r->n)) return -1;
    for (int i = 0; i < n; i++) { const SxRtpStream z = {0, 0, 0, 0}; r->cfg[(size_t)streams[i]] = z; }
    emu_clear(r, streams, n);
    sx_rtp_table(r->cfg, 0, r->table);
    return 0;
}
int emu_srtcp_set_keys(void* h, const int* streams, int n, const unsigned char* tx, const unsigned char* rx, const unsigned* tx_index, const long long* rx_index) {
    EmuSrtcp* r = (EmuSrtcp*)h;
    std::vector<SxSrtpKey> recs;
    std::vector<SxSrtcpTx> txs;
    std::vector<SxSrtcpRx> rxs;
    SxSrtcpMirror next;
    if (!r || !sx_srtcp_set_keys_plan(r->mirror, r->n, streams, n, tx, rx, tx_index, (const i64*)rx_index, next, recs, txs, rxs)) return -1;
    if (r->mem.empty()) {
        r->mem.resize(sx_srtcp_bytes(r->n));
        sx_srtcp_mem_init(r->mem.data(), r->n);
    }
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
int emu_srtcp_clear_keys(void* h, const int* streams, int n) {
    EmuSrtcp* r = (EmuSrtcp*)h;
    if (!r || !sx_list_ok(streams, n, r->n)) return -1;
    emu_clear(r, streams, n);
    return 0;
}
int emu_srtcp_get_index(void* h, const int* streams, int n, unsigned* tx_next, long long* rx_index) {
    EmuSrtcp* r = (EmuSrtcp*)h;
    if (!r || !sx_list_ok(streams, n, r->n)) return -1;
    const SxSrtcpMem m = emu_mem(r);
    for (int i = 0; i < n; i++) {
        if (tx_next) tx_next[i] = m.tx ? m.tx[streams[i]].next : 0u;
        if (rx_index) rx_index[i] = m.rx ? (long long)m.rx[streams[i]].index : -1;
    }
    return 0;
}
// everything the session keeps for SRTCP: the allocation's bytes, then the mirror (2 per stream) -> its size; out NULL: only the size
int emu_srtcp_snapshot(void* h, unsigned char* out) {
    EmuSrtcp* r = (EmuSrtcp*)h;
    const size_t a = r->mem.size(), b = r->mirror.has_tx.size();
    if (out) {
        if (a) memcpy(out, r->mem.data(), a);
        if (b) { memcpy(out + a, r->mirror.has_tx.data(), b); memcpy(out + a + b, r->mirror.has_rx.data(), b); }
    }
    return (int)(a + 2 * b);
}
// words of stream's two key records that are not zero
int emu_srtcp_key_words(void* h, int stream) {
    EmuSrtcp* r = (EmuSrtcp*)h;
    if (r->mem.empty()) return 0;
    int n = 0;
    const u32* w = (const u32*)(emu_mem(r).keys + 2 * (size_t)stream);
    for (int k = 0; k < 2 * SOLO_SRTP_KEY_WORDS; k++) n += w[k] != 0;
    return n;
}
int emu_srtcp_trailer_ok(int trailer) { return sx_srtcp_trailer_ok(trailer) ? 0 : -1; }

// ---- the calls ----------------------------------------------------------------------------------------------------------------------------------
// emu_rtcp_build of tests/rtcp_host.cpp with the trailer switch
int emu_srtcp_build(void* h, const unsigned* cfg_tx, int tx_streams, int packet_samples, const unsigned* cfg_rx, int rx_streams, const int* streams, int n,
                    unsigned long long now, void* dgrams, unsigned char* wire, long long cap, void* count, int trailer) {
    EmuRtcp* c = (EmuRtcp*)h;
    if (!cfg_tx || !sx_rtcp_build_ok(c, c ? c->n : 0, tx_streams, cfg_rx != NULL, rx_streams, streams, n, NULL, dgrams, wire, cap, count)) return -1;
    SxRtcpBuildArgs a = {};
    a.streams = streams; a.cfg_tx = (const SxRtpStream*)cfg_tx; a.cfg_rx = (const SxRtpStream*)cfg_rx; a.state = c->state.data(); a.cname = c->cname.data();
    a.d_now = NULL; a.now = now; a.dgrams = (SxRtpDgram*)dgrams; a.wire = wire; a.cap = cap; a.count = (SxRtcpBuildCount*)count;
    a.n = n; a.n_streams = c->n; a.packet_samples = packet_samples; a.trailer = trailer;
    return sx_rtcp_build_host(a) ? 0 : 1;
}
// rtcp_streams / trailer: what the call reads of the RTCP object.  -> -1: refused by the argument rules
int emu_srtcp_protect(void* h, int rtcp_streams, int trailer, const int* streams, int n, const void* build_count, void* dgrams, unsigned char* wire,
                      long long wire_bytes, void* count) {
    EmuSrtcp* r = (EmuSrtcp*)h;
    if (!sx_srtcp_protect_ok(rtcp_streams > 0 ? (const void*)r : NULL, rtcp_streams, trailer, r, r ? r->n : 0, streams, n, build_count, dgrams, wire, wire_bytes, count))
        return -1;
    const SxSrtcpMem m = emu_mem(r);
    SxSrtcpProtectArgs a;
    a.streams = streams; a.build_count = (const SxRtcpBuildCount*)build_count; a.dgrams = (SxRtpDgram*)dgrams; a.wire = wire; a.keys = m.keys; a.tx = m.tx;
    a.wire_bytes = wire_bytes > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : wire_bytes;
    a.n = n; a.n_streams = r->n;
    sx_srtcp_protect_host(a, (SxSrtcpCount*)count);
    return 0;
}
int emu_srtcp_unprotect(void* h, const void* dgrams, int n_dgrams, unsigned char* wire, long long wire_bytes, void* dgrams_out, void* count) {
    EmuSrtcp* r = (EmuSrtcp*)h;
    if (!sx_srtcp_unprotect_ok(r, dgrams, n_dgrams, wire, wire_bytes, dgrams_out, count)) return -1;
    const SxSrtcpMem m = emu_mem(r);
    SxSrtcpUnprotectArgs a;
    a.dgrams = (const SxRtpDgram*)dgrams; a.out = (SxRtpDgram*)dgrams_out; a.wire = wire; a.table = r->table.data(); a.keys = m.keys; a.rx = m.rx;
    a.wire_bytes = wire_bytes > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : wire_bytes;
    a.n_dgrams = n_dgrams; a.n_streams = r->n;
    sx_srtcp_unprotect_host(a, (SxSrtcpCount*)count);
    return 0;
}

}

#if defined(SRTCP_MAIN)
// in:  int32 {n_streams, n_dgrams, wire_bytes, 0, 0, 0, 0, 0}; uint32 ssrc [n_streams]; int64 rx index [n_streams]; uint8 rx master
//      [n_streams][30]; int32 dgrams [n_dgrams][2]; uint8 wire [wire_bytes]
// out: int32 dgrams_out [n_dgrams][2]; int32 count [8]; int64 rx index [n_streams]; uint8 wire [wire_bytes]
// Every buffer is a heap block of exactly its size, so a read or write one byte outside it is a report.
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[8];
    if (fread(hdr, 4, 8, f) != 8) return 2;
    const int N = hdr[0], n = hdr[1], wb = hdr[2];
    unsigned* ssrc = (unsigned*)malloc(4 * (size_t)N);
    long long* index = (long long*)malloc(8 * (size_t)N);
    unsigned char* master = (unsigned char*)malloc(30 * (size_t)N);
    int* dg = (int*)malloc(8 * (size_t)n);
    unsigned char* wire = (unsigned char*)malloc((size_t)wb);
    if (fread(ssrc, 4, (size_t)N, f) != (size_t)N || fread(index, 8, (size_t)N, f) != (size_t)N || fread(master, 30, (size_t)N, f) != (size_t)N ||
        fread(dg, 8, (size_t)n, f) != (size_t)n || fread(wire, 1, (size_t)wb, f) != (size_t)wb)
        return 2;
    fclose(f);
    unsigned* cfg = (unsigned*)calloc(4 * (size_t)N, 4);
    int* streams = (int*)malloc(4 * (size_t)N);
    for (int s = 0; s < N; s++) { streams[s] = s; cfg[4 * s] = ssrc[s]; cfg[4 * s + 3] = 1; }
    void* h = emu_srtcp_create(cfg, N);
    if (!h || emu_srtcp_set_keys(h, streams, N, NULL, master, NULL, index) != 0) return 3;
    int* out = (int*)malloc(8 * (size_t)n);
    int count[8];
    if (emu_srtcp_unprotect(h, dg, n, wire, wb, out, count) != 0) return 3;
    emu_srtcp_get_index(h, streams, N, NULL, index);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out, 8, (size_t)n, f); fwrite(count, 4, 8, f); fwrite(index, 8, (size_t)N, f); fwrite(wire, 1, (size_t)wb, f);
    fclose(f);
    emu_srtcp_destroy(h);
    free(ssrc); free(index); free(master); free(dg); free(wire); free(cfg); free(streams); free(out);
    return 0;
}
#endif

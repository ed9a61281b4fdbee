// Host build of the RTCP stage (solo_amd/csrc/solo_rtcp.h) for tests/test_rtcp_model.py, which compiles this file into a temporary
// directory through tests/host_build.py.  The object is the host mirror of solo_api.hip's: the rows and the CNAMEs in vectors, the same
// argument rules (sx_rtcp_*_ok, sx_rtcp_cname_ok, sx_list_ok) in front of the same passes.  A session is what the device code reads of
// a solo_rtp_t: its records (uint32 [n][4] = SxRtpStream) and the table sx_rtp_table makes of them.
// With -DRTCP_HOST_MAIN the file is a program of its own (a sanitizer build needs nothing else): a few ticks of every call.
#include <string.h>
#include "../solo_amd/csrc/solo_dec.h"
#include "../solo_amd/csrc/solo_rtcp.h"

struct EmuRtcp {
    int n;
    std::vector<SxRtcpRow> state;                           // [n]
    std::vector<u32> cname;                                 // [n][8]
};

extern "C" {

int emu_rtcp_sizes(int which) {
    return which == 0 ? (int)sizeof(SxRtcpRow) : which == 1 ? (int)sizeof(SxRtcpRecvCount) : which == 2 ? (int)sizeof(SxRtcpSentCount)
         : which == 3 ? (int)sizeof(SxRtcpBuildCount) : which == 4 ? (int)sizeof(SxRtcpParseCount) : which == 5 ? (int)sizeof(SxRtcpFeedback)
         : which == 6 ? SOLO_RTCP_STATE_BYTES : which == 7 ? SOLO_RTCP_CNAME_BYTES : SOLO_RTCP_WALK_MAX;
}
void* emu_rtcp_create(int n_streams) {
    if (n_streams <= 0) return NULL;
    EmuRtcp* c = new EmuRtcp();
    c->n = n_streams;
    c->state.resize((size_t)n_streams);
    memset(c->state.data(), 0, c->state.size() * sizeof(SxRtcpRow));
    c->cname.assign((size_t)n_streams * SX_RTCP_CNAME_WORDS, 0u);
    return c;
}
void emu_rtcp_destroy(void* h) { delete (EmuRtcp*)h; }
int emu_rtcp_reset_rows(void* h, const int* rows, int n) {
    EmuRtcp* c = (EmuRtcp*)h;
    if (!c || !sx_list_ok(rows, n, c->n)) return -1;
    for (int i = 0; i < n; i++) {
        memset(&c->state[(size_t)rows[i]], 0, sizeof(SxRtcpRow));
        memset(&c->cname[(size_t)rows[i] * SX_RTCP_CNAME_WORDS], 0, SOLO_RTCP_CNAME_BYTES);
    }
    return 0;
}
// the whole state as a blob, uint32 [n][32 + 8]: out (put = 0) or in
void emu_rtcp_state(void* h, unsigned* words, int put) {
    EmuRtcp* c = (EmuRtcp*)h;
    for (int s = 0; s < c->n; s++) {
        unsigned* w = words + (size_t)s * (SX_RTCP_WORDS + SX_RTCP_CNAME_WORDS);
        if (put) { memcpy(&c->state[s], w, sizeof(SxRtcpRow)); memcpy(&c->cname[(size_t)s * SX_RTCP_CNAME_WORDS], w + SX_RTCP_WORDS, SOLO_RTCP_CNAME_BYTES); }
        else { memcpy(w, &c->state[s], sizeof(SxRtcpRow)); memcpy(w + SX_RTCP_WORDS, &c->cname[(size_t)s * SX_RTCP_CNAME_WORDS], SOLO_RTCP_CNAME_BYTES); }
    }
}
int emu_rtcp_set_cname(void* h, const int* streams, int n, const char* names) {
    EmuRtcp* c = (EmuRtcp*)h;
    if (!c || !sx_rtcp_cname_ok(streams, n, names, c->n)) return -1;
    for (int i = 0; i < n; i++) memcpy(&c->cname[(size_t)streams[i] * SX_RTCP_CNAME_WORDS], names + (size_t)i * SOLO_RTCP_CNAME_BYTES, SOLO_RTCP_CNAME_BYTES);
    return 0;
}
// the device table of the records cfg [n][4]: table [4 + 2 n] words.  -> 0, or -1: an SSRC twice
int emu_rtcp_table(const unsigned* cfg, int n, unsigned* table) {
    std::vector<SxRtpStream> v((size_t)n);
    memcpy(v.data(), cfg, v.size() * sizeof(SxRtpStream));
    std::vector<u32> t;
    if (!sx_rtp_table(v, 0, t)) return -1;
    memcpy(table, t.data(), t.size() * sizeof(u32));
    return 0;
}
int emu_rtcp_received(void* h, const unsigned* cfg, int session_streams, int packet_samples, const void* arrivals, const unsigned short* rtp_seq, int n_dgrams,
                      const unsigned* arrival_time, unsigned now_rtp, void* count) {
    EmuRtcp* c = (EmuRtcp*)h;
    if (!cfg || !sx_rtcp_received_ok(c, c ? c->n : 0, session_streams, arrivals, rtp_seq, n_dgrams, arrival_time, count)) return -1;
    SxRtcpRecvArgs a = {};
    a.arrivals = (const SxSendRecord*)arrivals; a.rtp_seq = rtp_seq; a.arrival_time = arrival_time; a.cfg = (const SxRtpStream*)cfg; a.state = c->state.data();
    a.count = (i32*)count; a.now_rtp = now_rtp; a.n_dgrams = n_dgrams; a.n_streams = c->n; a.packet_samples = packet_samples;
    sx_rtcp_received_host(a);
    return 0;
}
int emu_rtcp_sent(void* h, int session_streams, const void* records, const void* send_count, int max_records, const void* dgrams, void* count) {
    EmuRtcp* c = (EmuRtcp*)h;
    if (!sx_rtcp_sent_ok(c, c ? c->n : 0, session_streams, records, send_count, max_records, dgrams, count)) return -1;
    SxRtcpSentArgs a;
    a.records = (const SxSendRecord*)records; a.send_count = (const SxSendCount*)send_count; a.dgrams = (const SxRtpDgram*)dgrams; a.state = c->state.data();
    a.count = (i32*)count; a.max_records = max_records; a.n_streams = c->n;
    sx_rtcp_sent_host(a);
    return 0;
}
// -> -1: refused by the argument rules; 0: done; 1: refused by the list (built = -1)
int emu_rtcp_build(void* h, const unsigned* cfg_tx, int tx_streams, int packet_samples, const unsigned* cfg_rx, int rx_streams, const int* streams, int n,
                   unsigned long long now, const unsigned long long* p_now, void* dgrams, unsigned char* wire, long long cap, void* count) {
    EmuRtcp* c = (EmuRtcp*)h;
    if (!cfg_tx || !sx_rtcp_build_ok(c, c ? c->n : 0, tx_streams, cfg_rx != NULL, rx_streams, streams, n, p_now, dgrams, wire, cap, count)) return -1;
    SxRtcpBuildArgs a = {};
    a.streams = streams; a.cfg_tx = (const SxRtpStream*)cfg_tx; a.cfg_rx = (const SxRtpStream*)cfg_rx; a.state = c->state.data(); a.cname = c->cname.data();
    a.d_now = p_now; a.now = now; a.dgrams = (SxRtpDgram*)dgrams; a.wire = wire; a.cap = cap; a.count = (SxRtcpBuildCount*)count;
    a.n = n; a.n_streams = c->n; a.packet_samples = packet_samples;
    return sx_rtcp_build_host(a) ? 0 : 1;
}
int emu_rtcp_parse(void* h, const unsigned* table_rx, int rx_streams, const unsigned* table_tx, int tx_streams, const void* dgrams, int n_dgrams,
                   const unsigned char* wire, long long wire_bytes, unsigned long long now, const unsigned long long* p_now, void* feedback, void* count) {
    EmuRtcp* c = (EmuRtcp*)h;
    if (!table_rx || !sx_rtcp_parse_ok(c, c ? c->n : 0, rx_streams, table_tx != NULL, tx_streams, dgrams, n_dgrams, wire, wire_bytes, p_now, feedback, count))
        return -1;
    SxRtcpParseArgs a = {};
    a.dgrams = (const SxRtpDgram*)dgrams; a.wire = wire; a.table_rx = table_rx; a.table_tx = table_tx; a.state = c->state.data();
    a.feedback = (SxRtcpFeedback*)feedback; a.count = (i32*)count; a.d_now = p_now; a.now = now;
    a.wire_bytes = wire_bytes > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : wire_bytes;
    a.n_dgrams = n_dgrams; a.n_streams = c->n;
    sx_rtcp_parse_host(a);
    return 0;
}

}

#ifdef RTCP_HOST_MAIN
#include <stdio.h>
// two objects A and B of N streams; A receives 3 x N + 300 datagrams a tick (one stream floods), sends, builds; B parses and builds; A parses
int main() {
    const int N = 70, L = 640, TICKS = 6;
    std::vector<unsigned> cfg_a(4 * N), cfg_b(4 * N), tab_a(4 + 2 * N), tab_b(4 + 2 * N);
    for (int s = 0; s < N; s++) {
        const unsigned a[4] = {0x1000u + (unsigned)s * 7u, 0xFFFF0000u + (unsigned)s, 65530u | (96u << 16) | (97u << 24), 1u};
        const unsigned b[4] = {0x900000u - (unsigned)s * 3u, 123u * (unsigned)s, (unsigned)s | (96u << 16) | (97u << 24), 1u};
        memcpy(&cfg_a[4 * s], a, 16); memcpy(&cfg_b[4 * s], b, 16);
    }
    if (emu_rtcp_table(cfg_a.data(), N, tab_a.data()) || emu_rtcp_table(cfg_b.data(), N, tab_b.data())) return 1;
    void* A = emu_rtcp_create(N);
    void* B = emu_rtcp_create(N);
    std::vector<int> all(N);
    std::vector<char> names((size_t)N * 32, 0);
    for (int s = 0; s < N; s++) { all[s] = s; snprintf(&names[(size_t)s * 32], 32, "peer%d@host", s); }
    if (emu_rtcp_set_cname(A, all.data(), N, names.data()) || emu_rtcp_set_cname(B, all.data(), N, names.data())) return 2;
    long long sum = 0;
    for (int t = 0; t < TICKS; t++) {
        const int nd = 3 * N + 300;
        std::vector<int> arr(5 * (size_t)nd), recs(5 * (size_t)nd), dg(2 * (size_t)nd);
        std::vector<unsigned short> seq(nd);
        std::vector<unsigned> at(nd);
        for (int i = 0; i < nd; i++) {
            const int s = i < 3 * N ? i % N : 5, q = t * 400 + i / N;
            const int rec[5] = {i % 11 == 10 ? -1 : s, q, i & 1, 0, 40};
            memcpy(&arr[5 * (size_t)i], rec, 20); memcpy(&recs[5 * (size_t)i], rec, 20);
            seq[i] = (unsigned short)(65530 + 2 * q + (i & 1) + (i % 13 == 0 ? 3500 : 0));
            at[i] = 0xFFFFF000u + (unsigned)(t * 640 + (i * 37) % 500);
            dg[2 * (size_t)i] = 64 * i; dg[2 * (size_t)i + 1] = i % 5 == 4 ? 0 : 52;
        }
        int cnt[16], sc[8] = {nd, nd, 0, 0, 0, 0, 0, 0};
        if (emu_rtcp_received(A, cfg_b.data(), N, L, arr.data(), seq.data(), nd, t & 1 ? at.data() : NULL, 0x100u * (unsigned)t, cnt)) return 3;
        sum += cnt[0] + 3 * cnt[4];
        if (emu_rtcp_sent(A, N, recs.data(), sc, nd, dg.data(), cnt)) return 4;
        sum += cnt[0];
        std::vector<unsigned char> wire(96 * (size_t)N + 3), wire2(96 * (size_t)N);
        std::vector<int> out(2 * (size_t)N), fb(8 * (size_t)N);
        long long bc[4];
        const unsigned long long now = (0x83AA7E80ull + (unsigned)t) << 32;
        if (emu_rtcp_build(A, cfg_a.data(), N, L, cfg_b.data(), N, all.data(), N, now, NULL, out.data(), wire.data(), 96 * N, bc)) return 5;
        if (emu_rtcp_parse(B, tab_a.data(), N, tab_b.data(), N, out.data(), N, wire.data() + (t & 1), 96 * N, now + 0x8000, NULL, fb.data(), cnt)) return 6;
        sum += cnt[0] + cnt[4];
        if (emu_rtcp_build(B, cfg_b.data(), N, L, cfg_a.data(), N, all.data(), N, now + (3ull << 32), NULL, out.data(), wire2.data(), 50 * N, bc)) return 7;
        if (emu_rtcp_parse(A, tab_b.data(), N, tab_a.data(), N, out.data(), N, wire2.data(), 50 * N, now + (4ull << 32), NULL, fb.data(), cnt)) return 8;
        sum += cnt[0] + fb[7];
    }
    emu_rtcp_destroy(A);
    emu_rtcp_destroy(B);
    printf("rtcp host ok %lld\n", sum);
    return 0;
}
#endif

// Host build of the read side of the receiver ring (solo_amd/csrc/solo_recv_report.h) for tests/test_recv_report_model.py, which
// compiles this file into a temporary directory through tests/host_build.py.
#include <string.h>
#include "../solo_amd/csrc/solo_dec.h"
#include "../solo_amd/csrc/solo_recv_report.h"

extern "C" {

int emu_recv_report_size() { return (int)sizeof(SxRecvReport); }
int emu_recv_report_count_size() { return (int)sizeof(SxRecvReportCount); }
int emu_recv_trk_words() { return SX_RECV_TRK_WORDS; }
int emu_recv_group(int depth) { return sx_recv_group(depth); }
int emu_recv_play_class(unsigned int lw) { return sx_recv_play_class(lw); }
int emu_recv_select(int ready, int span, int m, int max_span) { return sx_recv_select(ready, span, m, max_span); }

// the report and the compaction over n rows -> number of selected rows; sel: int [n] of scratch
int emu_recv_report(const unsigned int* lens, const int* play, unsigned int* trk, const int* map, const int* min_ready_v, int n, int depth,
                    int min_ready, int max_span, int clear_margin, unsigned int* reports, int* sel, int* list, int* rows) {
    SxRecvReportArgs a;
    a.lens = lens; a.play = play; a.trk = trk; a.map = map; a.min_ready_v = min_ready_v; a.reports = reports; a.sel = sel;
    a.n = n; a.depth = depth; a.min_ready = min_ready; a.max_span = max_span; a.clear_margin = clear_margin;
    return sx_recv_report_host(a, list, rows);
}

}

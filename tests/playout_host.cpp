// Host build of the play-out delay control (solo_amd/csrc/solo_playout.h) for tests/test_playout_model.py and tests/test_playout_abi.py,
// which compile this file into a temporary directory through tests/host_build.py.  An "object" here is the caller's
// memory: state int32 [n_rows][32], held int16 [n_rows][L], slot / sslot int32 [n_rows].
#include <string.h>
#include "../solo_amd/csrc/solo_playout.h"

extern "C" {

int emu_po_params_size() { return (int)sizeof(SxPoParams); }
int emu_po_plan_count_size() { return (int)sizeof(SxPoPlanCount); }
int emu_po_render_count_size() { return (int)sizeof(SxPoRenderCount); }
int emu_po_count_size() { return (int)sizeof(SxPoCount); }
int emu_po_state_bytes() { return SX_PO_STATE_WORDS * 4; }
int emu_po_blob_row_bytes(int L) { return (int)(sx_po_blob_row_words(L) * 4); }
int emu_po_params_ok(const SxPoParams* p) { return sx_po_params_ok(p); }
int emu_po_geometry_ok(int n_rows, int L) { return sx_po_geometry_ok(n_rows, L); }
int emu_po_list_ok(const int* rows, int n, int n_rows) { return sx_po_list_ok(rows, n, n_rows); }
int emu_po_tick_call_ok(int n_rows, int L, int ring, int tracking, int h_streams, int h_depth, int h_L, int h_fs, const void* rows, int n, const SxPoParams* p,
                        const void* heard, const void* outcome, const void* status, const void* count) {
    return sx_po_tick_call_ok(n_rows, L, ring != 0, tracking != 0, h_streams, h_depth, h_L, h_fs, rows, n, p, heard, outcome, status, count);
}

// -> 0, -1 when the call is refused on the host (nothing written), 1 when the list is refused "on the device" (count->n_one = -1 only)
int emu_po_plan(int* state, int n_rows, int* slot, int* sslot, const unsigned* reports, const int* rows, int n, int depth, const SxPoParams* p, int* action,
                int* one, int* two, int* spos, SxPoPlanCount* count) {
    if (!sx_po_plan_call_ok(n_rows, reports, rows, n, depth, p, action, one, two, spos, count)) return -1;
    SxPoPlanArgs a;
    a.reports = reports; a.state = state; a.map = rows; a.action = action; a.p = *p; a.n = n; a.depth = depth;
    return sx_po_plan_host(a, n_rows, one, two, spos, slot, sslot, count) ? 0 : 1;
}

int emu_po_gather(int n_rows, const short* pcm_one, int n_one, const int* spos, int n_stretch, int L, short* out) {
    if (!sx_po_gather_call_ok(n_rows, pcm_one, n_one, spos, n_stretch, out)) return -1;
    sx_po_gather_host(pcm_one, spos, n_one, n_stretch, L, out);
    return 0;
}

int emu_po_render(int* state, short* held, int n_rows, int L, const int* slot, const int* sslot, const int* rows, int n, const SxPoParams* p, int block,
                  const int* action, int n_one, int n_two, int n_stretch, const short* pcm_one, const int* st_one, const short* pcm_two, const int* st_two,
                  const short* ts_s, const int* cost_s, const short* ts_a, const int* cost_a, short* heard, int* outcome, int* status, SxPoRenderCount* count) {
    if (!sx_po_render_call_ok(n_rows, L, rows, n, p, block, action, n_one, n_two, n_stretch, pcm_one, st_one, pcm_two, st_two, ts_s, cost_s, ts_a, cost_a, heard,
                              outcome, status, count))
        return -1;
    SxPoRenderArgs a;
    a.state = state; a.held = held; a.map = rows; a.action = action; a.slot = slot; a.sslot = sslot;
    a.pcm_one = pcm_one; a.st_one = st_one; a.pcm_two = pcm_two; a.st_two = st_two; a.ts_s = ts_s; a.cost_s = cost_s; a.ts_a = ts_a; a.cost_a = cost_a;
    a.heard = heard; a.outcome = outcome; a.status = status;
    a.n = n; a.n_one = n_one; a.n_two = n_two; a.n_stretch = n_stretch; a.L = L; a.M = L / block; a.cooldown = p->cooldown; a.cost_gate = p->cost_gate;
    return sx_po_render_host(a, n_rows, count) ? 0 : 1;
}

}

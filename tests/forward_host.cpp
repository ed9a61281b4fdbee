// Host build of the forwarding stage (solo_amd/csrc/solo_forward.h) for tests/test_forward_model.py, which compiles this file into a
// temporary directory through tests/host_build.py.  The object is the host mirror of solo_api.hip's: the state records in a vector, the
// same argument rules (sx_fwd_levels_ok, sx_fwd_route_ok, sx_list_ok) in front of the same passes.
#include <string.h>
#include "../solo_amd/csrc/solo_dec.h"
#include "../solo_amd/csrc/solo_forward.h"

struct EmuForward {
    int n_rows, K;
    std::vector<SxFwdSlot> state;                           // [n_rows][K]
};
static void emu_reset_room(EmuForward* f, int r) {
    for (int w = 0; w < f->K * SX_FWD_SLOT_WORDS; w++) ((i32*)&f->state[(size_t)r * f->K])[w] = sx_fwd_init_word(w);
}

extern "C" {

int emu_forward_sizes(int which) {
    return which == 0 ? (int)sizeof(SxFwdRow) : which == 1 ? (int)sizeof(SxFwdCount) : which == 2 ? (int)sizeof(SxFwdSlot) : (int)SOLO_FORWARD_STATE_BYTES(3);
}
void* emu_forward_create(int n_rows, int slots) {
    if (n_rows <= 0 || slots < 1 || slots > SX_FWD_MAX_SLOTS) return NULL;
    EmuForward* f = new EmuForward();
    f->n_rows = n_rows; f->K = slots;
    f->state.resize((size_t)n_rows * slots);
    for (int r = 0; r < n_rows; r++) emu_reset_room(f, r);
    return f;
}
void emu_forward_destroy(void* h) { delete (EmuForward*)h; }
int emu_forward_reset_rooms(void* h, const int* rooms, int n) {
    EmuForward* f = (EmuForward*)h;
    if (!f || !sx_list_ok(rooms, n, f->n_rows)) return -1;
    for (int i = 0; i < n; i++) emu_reset_room(f, rooms[i]);
    return 0;
}
// the whole state, int32 [n_rows][4 K]: out (put = 0) or in
void emu_forward_state(void* h, int* words, int put) {
    EmuForward* f = (EmuForward*)h;
    if (put) memcpy(f->state.data(), words, f->state.size() * sizeof(SxFwdSlot));
    else memcpy(words, f->state.data(), f->state.size() * sizeof(SxFwdSlot));
}
int emu_forward_levels(const void* arrivals, const unsigned char* level_in, int n_dgrams, int n_rows, int default_level, void* rowinfo, unsigned char* sa,
                       unsigned char* level) {
    if (!sx_fwd_levels_ok(arrivals, n_dgrams, n_rows, default_level, rowinfo, sa, level)) return -1;
    SxFwdLevelArgs a;
    a.arrivals = (const SxSendRecord*)arrivals; a.level_in = level_in; a.rowinfo = (SxFwdRow*)rowinfo; a.sa = sa; a.level = level;
    a.n_dgrams = n_dgrams; a.n_rows = n_rows; a.default_level = default_level;
    sx_fwd_levels_host(a);
    return 0;
}
// -> -1: refused by the argument rules; 0: done; 1: refused by the room ids (the two marks written)
int emu_forward_route(void* h, const void* arrivals, int n_dgrams, const void* rowinfo, const unsigned char* sel, const int* room, int n, int n_rooms,
                      void* records, int max_records, void* send_count, unsigned char* level_fwd, int* slot_src, void* count) {
    EmuForward* f = (EmuForward*)h;
    if (!sx_fwd_route_ok(f, f ? f->n_rows : 0, arrivals, n_dgrams, rowinfo, sel, room, n, n_rooms, records, max_records, send_count, slot_src, count)) return -1;
    SxFwdArgs a = {};
    a.arrivals = (const SxSendRecord*)arrivals; a.rowinfo = (const SxFwdRow*)rowinfo; a.sel = sel; a.room = room; a.state = f->state.data();
    a.records = (SxSendRecord*)records; a.send_count = (SxSendCount*)send_count; a.level_fwd = level_fwd; a.slot_src = slot_src; a.count = (SxFwdCount*)count;
    a.n_dgrams = n_dgrams; a.n = n; a.n_rooms = n_rooms; a.K = f->K; a.max_records = max_records;
    return sx_fwd_route_host(a, f->n_rows) ? 0 : 1;
}

}

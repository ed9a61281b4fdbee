// Host build of the stream migration (solo_amd/csrc/solo_migrate.h: export, check and import in their host forms) for
// tests/test_migrate_model.py, which compiles this file into a temporary directory through tests/host_build.py.
#include <string.h>
#include "../solo_amd/csrc/solo_dec.h"          // (the tables solo_recv.h reads)
#include "../solo_amd/csrc/solo_migrate.h"

static SxMigHandle emu_handle(unsigned char* enc, unsigned char* dec, unsigned char* ring, unsigned int* lens, int* play, unsigned int* trk, const int* geom8,
                              int n_streams) {
    SxMigHandle h;
    h.enc = enc; h.dec = dec; h.ring = ring; h.lens = lens; h.play = play; h.trk = trk;
    memcpy(&h.g, geom8, sizeof(h.g));
    h.n_streams = n_streams;
    return h;
}

extern "C" {

int emu_mig_count_size() { return (int)sizeof(SxMigCount); }
int emu_mig_geom_size() { return (int)sizeof(SxMigGeom); }

long long emu_mig_state_bytes(const int* geom8, int which) {
    SxMigGeom g;
    memcpy(&g, geom8, sizeof(g));
    return SX_MIG_HDR_BYTES + sx_mig_body_bytes(sx_mig_geom_of(g, which), which);
}

void emu_mig_export(unsigned char* enc, unsigned char* dec, unsigned char* ring, unsigned int* lens, int* play, unsigned int* trk, const int* geom8, int n_streams,
                    const int* map, int n, int which, unsigned char* blob, long long stride, void* count) {
    sx_mig_export_host(emu_handle(enc, dec, ring, lens, play, trk, geom8, n_streams), map, n, which, blob, stride, (SxMigCount*)count);
}

// returns the reason the first bad record was refused for (0: imported)
int emu_mig_import(unsigned char* enc, unsigned char* dec, unsigned char* ring, unsigned int* lens, int* play, unsigned int* trk, const int* geom8, int n_streams,
                   const int* map, int n, int which, const unsigned char* blob, long long stride, void* count) {
    int why = 0;
    sx_mig_import_host(emu_handle(enc, dec, ring, lens, play, trk, geom8, n_streams), map, n, which, blob, stride, (SxMigCount*)count, &why);
    return why;
}

// both sums over n_quads x 4 words (16-byte aligned), as the kernels accumulate them
void emu_mig_sums(const unsigned char* body, long long n_quads, unsigned int* out2) {
    SxMigSum a;
    a.s1 = 0u; a.s2 = 0u;
    for (long long q = 0; q < n_quads; q++) sx_mig_acc(&a, (u32)(4 * q), ((const SxMigQ*)body)[q]);
    out2[0] = a.s1; out2[1] = a.s2;
}

}

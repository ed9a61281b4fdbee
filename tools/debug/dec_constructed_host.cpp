// Stand-alone host run of the decoder source over a list of payloads, for a sanitizer build (never loaded into python, never run on the GPU):
// the extraction step (sx_extract_desc) with guard bytes on both sides of the lane's byte row -- an overflow inside a struct is invisible to
// ASan --, then sx_decode_packet from the extraction's records and without records.  Every payload sits in a heap block of its own length
// + 8 (the slack a batch slot has behind its longest record), so a read beyond it is reported.
//
//   python tools/debug/dec_constructed_dump.py /tmp/dc             (writes /tmp/dc_nb.bin and /tmp/dc_wb.bin from tests/golden/dec_constructed*.npz)
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fwrapv -fno-strict-aliasing -DSOLO_HOST_EMU \
//       tools/debug/dec_constructed_host.cpp -o /tmp/dc_host_nb && /tmp/dc_host_nb /tmp/dc_nb.bin
//   (the 32 kHz API rate: add -DSX_FS_KHZ=16, run on /tmp/dc_wb.bin)
// File: per stream int32 (flags of emu_dec_create, packets), per packet int32 (nBytes0, nBytes1, lostflag, bytes handed over) and the bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "../../solo_amd/csrc/solo_dec.h"

struct Dec { SxDecState st; SxDecWork w; SxDecShadow sh; };
struct Guarded { u8 before[64]; SxExtractLane L; u8 after[64]; };

static Dec* dec_new(int flags) {
    Dec* d = (Dec*)calloc(1, sizeof(Dec));
    sx_dec_state_init(&d->st, ((flags >> 1) & 1) | (((flags >> 3) & 1) << 1));
    return d;
}
static int dec_packet(Dec* d, const u8* bits, int a0, int a1, int lf, int md, const SxExtracted* ext2, int16_t* pcm) {
    sx_cdf_load_dec(&d->w.cdf);
    d->w.st = d->st;
    d->w.shadow = &d->sh;
    const int r = sx_decode_packet(&d->w, bits, a0, a1, lf, md, pcm, ext2);
    d->st = d->w.st;
    return r;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s payloads.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hd[2];
    long streams = 0, packets = 0, taken = 0, differ = 0;
    Guarded* G = (Guarded*)malloc(sizeof(Guarded));
    while (fread(hd, 4, 2, f) == 2) {
        const int flags = hd[0], P = hd[1], md = flags & 1;
        Dec *a = dec_new(flags), *b = dec_new(flags);
        int16_t *pa = (int16_t*)malloc(SX_PACKET * 2), *pb = (int16_t*)malloc(SX_PACKET * 2);
        for (int p = 0; p < P; p++) {
            int32_t q[4];
            if (fread(q, 4, 4, f) != 4) return 2;
            const int a0 = q[0], a1 = q[1], lf = q[2], n = q[3];
            u8* bits = (u8*)calloc(1, (size_t)n + 8);
            if (n && fread(bits, 1, (size_t)n, f) != (size_t)n) return 2;
            SxExtracted* ext2 = (SxExtracted*)calloc(2, sizeof(SxExtracted));
            memset(G->before, 0xC3, sizeof(G->before));
            memset(G->after, 0xC3, sizeof(G->after));
            sx_cdf_load_dec(&a->w.cdf);
            const int hb_joint = a->st.hb_joint | (a->st.fpp == 1);
            for (int k = 0; k < 2; k++) {
                i32 off = 0, len = 0, hb_off = -1;
                int sel = 0;
                if (sx_desc_span(lf, a0, a1, hb_joint, k, &off, &len, &sel, &hb_off))
                    sx_extract_desc(bits + off, len, md, (const SxCdf*)&a->w.cdf, &G->L, &ext2[k], sel, hb_off >= 0 ? bits + hb_off : 0, hb_joint);
            }
            for (size_t i = 0; i < sizeof(G->before); i++)
                if (G->before[i] != 0xC3 || G->after[i] != 0xC3) { fprintf(stderr, "stream %ld packet %d: the lane's row ran over its guard bytes\n", streams, p); return 1; }
            taken += lf >= 2 && sx_extracted_usable(&a->st, ext2, lf);
            const int ra = dec_packet(a, bits, a0, a1, lf, md, ext2, pa);
            const int rb = dec_packet(b, bits, a0, a1, lf, md, 0, pb);
            if (ra != rb || (ra == 0 && memcmp(pa, pb, SX_PACKET * 2))) differ++;
            free(ext2);
            free(bits);
            packets++;
        }
        free(pa); free(pb); free(a); free(b);
        streams++;
    }
    free(G);
    fclose(f);
    printf("%ld streams, %ld packets, %ld through the records, %ld packets on which the two paths differ\n", streams, packets, taken, differ);
    return differ ? 1 : 0;
}

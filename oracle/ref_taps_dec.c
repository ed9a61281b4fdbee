/* Test infrastructure only: stage taps for the compiled reference DECODER (tests/golden/make_dec_stages.py, tests/test_dec_stages.py).
 *
 * Linked into oracle/_ref/libsolo_ref_fix_taps.so next to oracle/ref_taps.c, with -Wl,--wrap=<function> for each function named below
 * (oracle/Makefile: WRAP).  Every wrapper calls the real, unmodified function and records, as int32, what went in or came out:
 *
 *   solo_dec_tap_rec   one record per SKP_Silk_decode_parameters call (SKP_Silk_decode_frame.c:104, :107: per low-band decoder call and
 *                      per description): the symbols in the field order of the build's SxFrameSyms, the pulses, the de-quantised control
 *                      block in the order of SxDecCtrl, LastGainIndex afterwards and the prediction coefficients as SKP_Silk_NLSF2A_stable
 *                      returned them (SKP_Silk_decode_parameters.c:110, :121: before the expansion after a loss of line 134)
 *   solo_dec_tap_lo    the low band of every SKP_Silk_decode_frame call as it returns it
 *   solo_dec_tap_hb    per high-band frame (AGR_Bwe_decode_frame_FIX, AGR_BWE_decode_frame_FIX.c:40; the function is called from its own
 *                      file, so its callees are wrapped): the quantised LSPs, their prediction coefficients, the four sub-frame gains
 *   solo_dec_tap_hi    the synthesised high band
 *   solo_dec_tap_qmf   the two inputs of AGR_Sate_qmf_synth
 *   solo_dec_tap_state after every AGR_Sate_decode_process call (the body of AGR_Sate_Decoder_Decode, AGR_BWE_SDK_API.c:271): the return
 *                      code, then the live fields of the decoder, PLC, CNG and high-band state in the order of the build's SxDecState,
 *                      the QMF memories in time order (oldest sample first)
 * What the reference never assigns is recorded as zero.  The record sizes follow solo_dec_tap_fs (the internal rate of the run: 8 or 16),
 * which the caller sets together with solo_dec_tap_reset().  Nothing here is part of the product. */
#include <string.h>
#include "SKP_Silk_main.h"
#include "AGR_BWE_main_FIX.h"

#define DREC_INTS 512
#define DREC_MAX 160
#define DREC_SYMS 8
#define DREC_PULSES 96
#define DREC_CTL 416
#define DREC_A 454
#define DSTATE_INTS 4096
#define DPK_MAX 40
int solo_dec_tap_fs = 8;
int solo_dec_tap_n = 0, solo_dec_tap_syms = 0;
int solo_dec_tap_rec[DREC_MAX][DREC_INTS];
int solo_dec_tap_state_n = 0, solo_dec_tap_state_ints = 0;
int solo_dec_tap_state[DPK_MAX][DSTATE_INTS];
int solo_dec_tap_lo_n = 0, solo_dec_tap_hb_n = 0, solo_dec_tap_hi_n = 0, solo_dec_tap_qmf_n = 0;
short solo_dec_tap_lo[DPK_MAX * 2 * 320];
int solo_dec_tap_hb[DPK_MAX * 2][20];              /* lsp[8], lpc[8], gain[4] */
short solo_dec_tap_hi[DPK_MAX * 640];
short solo_dec_tap_qmf[DPK_MAX][2][640];
void solo_dec_tap_reset(int fs_kHz) {
    solo_dec_tap_fs = fs_kHz;
    solo_dec_tap_n = solo_dec_tap_state_n = solo_dec_tap_lo_n = solo_dec_tap_hb_n = solo_dec_tap_hi_n = solo_dec_tap_qmf_n = 0;
    memset(solo_dec_tap_rec, 0, sizeof(solo_dec_tap_rec));
    memset(solo_dec_tap_state, 0, sizeof(solo_dec_tap_state));
    memset(solo_dec_tap_hb, 0, sizeof(solo_dec_tap_hb));
}

static int *put(int *p, const void *src, int n, int elem) {
    int i;
    for (i = 0; i < n; i++) {
        if (elem == 4) *p++ = ((const int *)src)[i];
        else *p++ = ((const short *)src)[i];
    }
    return p;
}

/* ---- the symbols: every value the range decoder hands to SKP_Silk_decode_parameters itself (not to the pulse decoder) ---- */
static int in_params = 0, in_pulses = 0, n_sym = 0, sym[64], n_multi = 0, multi[16], n_a = 0;
static short a_out[2][16];
void __real_SKP_Silk_range_decoder(SKP_int *, SKP_Silk_range_coder_state *, const SKP_uint16 *, SKP_int);
void __wrap_SKP_Silk_range_decoder(SKP_int data[], SKP_Silk_range_coder_state *psRC, const SKP_uint16 prob[], SKP_int probIx) {
    __real_SKP_Silk_range_decoder(data, psRC, prob, probIx);
    if (in_params && !in_pulses && n_sym < 64) sym[n_sym++] = data[0];
}
void __real_SKP_Silk_range_decoder_multi(SKP_int *, SKP_Silk_range_coder_state *, const SKP_uint16 *const *, const SKP_int *, const SKP_int);
void __wrap_SKP_Silk_range_decoder_multi(SKP_int data[], SKP_Silk_range_coder_state *psRC, const SKP_uint16 *const prob[], const SKP_int probStartIx[],
                                         const SKP_int nSymbols) {
    int k;
    __real_SKP_Silk_range_decoder_multi(data, psRC, prob, probStartIx, nSymbols);
    if (in_params && !in_pulses)
        for (k = 0; k < nSymbols && k < 16; k++) multi[n_multi++] = data[k];
}
void __real_SKP_Silk_decode_pulses(SKP_Silk_range_coder_state *, SKP_Silk_decoder_control *, SKP_int *, const SKP_int);
void __wrap_SKP_Silk_decode_pulses(SKP_Silk_range_coder_state *psRC, SKP_Silk_decoder_control *psDecCtrl, SKP_int q[], const SKP_int frame_length) {
    in_pulses = 1;
    __real_SKP_Silk_decode_pulses(psRC, psDecCtrl, q, frame_length);
    in_pulses = 0;
}
void __real_SKP_Silk_NLSF2A_stable(SKP_int16 *, const SKP_int *, const SKP_int);
void __wrap_SKP_Silk_NLSF2A_stable(SKP_int16 pAR_Q12[], const SKP_int pNLSF[], const SKP_int LPC_order) {
    __real_SKP_Silk_NLSF2A_stable(pAR_Q12, pNLSF, LPC_order);
    if (in_params && n_a < 2) memcpy(a_out[n_a++], pAR_Q12, sizeof(short) * (size_t)LPC_order);
}

void __real_SKP_Silk_decode_parameters(SKP_Silk_decoder_state *, SKP_Silk_decoder_control *, SKP_int *, SKP_int, const SKP_int);
void __wrap_SKP_Silk_decode_parameters(SKP_Silk_decoder_state *psDec, SKP_Silk_decoder_control *c, SKP_int q[], SKP_int kDesp, const SKP_int fullDecoding) {
    const int f = psDec->nFramesDecoded, lossCnt = psDec->lossCnt, ffar = psDec->first_frame_after_reset, md = psDec->writeMDIndex == 1;
    int *r, *p, i, stages, lpc, voiced, complete;
    SKP_Silk_range_coder_state *psRC = &psDec->sMD[kDesp].sRC;
    in_params = 1; n_sym = n_multi = n_a = 0;
    memset(a_out, 0, sizeof(a_out));
    __real_SKP_Silk_decode_parameters(psDec, c, q, kDesp, fullDecoding);
    in_params = 0;
    if (solo_dec_tap_n >= DREC_MAX) return;
    r = solo_dec_tap_rec[solo_dec_tap_n++];
    memset(r, 0, sizeof(int) * DREC_INTS);
    lpc = solo_dec_tap_fs == 8 ? 10 : 16;
    stages = solo_dec_tap_fs == 8 ? 6 : 10;
    r[0] = f; r[1] = kDesp; r[2] = lossCnt; r[3] = ffar; r[5] = psDec->fs_kHz; r[6] = psDec->moreInternalDecoderFrames;
    /* the frame went through to its end when the symbols up to the frame termination were read: the head (index, rate: first frame only), type,
     * four gains (+ the description's gain ratio in the first frame), interpolation factor, (voiced: lag, contour, PER, four LTP, scale), seed,
     * VAD flag, termination */
    p = r + DREC_SYMS;
    i = 0;
    {
        int head = f == 0 ? md + 1 : 0, fs_ix = 0;
        if (f == 0) {
            if (md) p[1] = sym[i++];
            fs_ix = sym[i++];
            if (fs_ix < 0 || fs_ix > 3 || SKP_Silk_SamplingRates_table[fs_ix] != solo_dec_tap_fs) { p[0] = 1; complete = 0; goto tail; }
        }
        p[2] = sym[i++];
        voiced = (p[2] >> 1) == 0;
        p[3] = sym[i++]; p[4] = sym[i++]; p[5] = sym[i++]; p[6] = sym[i++];
        if (f == 0) p[7] = sym[i++];
        memcpy(p + 8, multi, sizeof(int) * (size_t)stages);
        p += 8 + stages;
        *p++ = sym[i++];                                        /* the interpolation factor as coded (the control block's may be overridden) */
        p = put(p, psDec->sMD[kDesp].prevNLSF_Q15, lpc, 4);     /* = pNLSF_Q15 of the frame (SKP_Silk_decode_parameters.c:128) */
        if (voiced) { memcpy(p, sym + i, sizeof(int) * 8); i += 8; }
        p += 8;
        *p++ = sym[i++];                                        /* Seed */
        *p++ = c->RateLevelIndex;
        *p++ = sym[i++]; *p++ = sym[i++];                       /* vadFlag, FrameTermination */
        complete = i == n_sym && i == head + 1 + 4 + (f == 0) + 1 + (voiced ? 8 : 0) + 3;
        (void)head;
    }
tail:
    p = r + DREC_SYMS + (solo_dec_tap_fs == 8 ? 40 : 50) - 3;
    p[0] = complete ? psDec->nBytesLeft[kDesp] : 0; p[1] = psRC->error; p[2] = psRC->bufferLength;
    solo_dec_tap_syms = (solo_dec_tap_fs == 8 ? 40 : 50);
    r[4] = complete;
    if (!complete) return;
    put(r + DREC_PULSES, q, psDec->frame_length <= 320 ? psDec->frame_length : 320, 4);
    p = r + DREC_CTL;
    p = put(p, c->pitchL, 4, 4); p = put(p, c->Gains_Q16, 4, 4); *p++ = c->DeltaGains_Q16; *p++ = c->Seed;
    p = put(p, c->LTPCoef_Q14, 20, 2); *p++ = c->LTP_scale_Q14;
    *p++ = c->PERIndex; *p++ = c->RateLevelIndex; *p++ = c->QuantOffsetType; *p++ = c->sigtype;
    *p++ = (f == 0 && md) ? c->MDIndex : 0;                     /* assigned in a packet's first frame alone, and only with writeMDIndex */
    *p++ = c->NLSFInterpCoef_Q2;
    *p++ = psDec->sMD[kDesp].LastGainIndex;
    p = r + DREC_A;
    *p++ = n_a;
    p = put(p, a_out[0], 16, 2);                                /* PredCoef_Q12[1]: the frame's own vector */
    p = put(p, a_out[1], 16, 2);                                /* PredCoef_Q12[0]: the interpolated one, if there was one */
}

SKP_int __real_SKP_Silk_decode_frame(SKP_Silk_decoder_state *, SKP_int16 *, SKP_int16 *, const SKP_uint8 *, const SKP_int16 *, SKP_int, SKP_int *);
SKP_int __wrap_SKP_Silk_decode_frame(SKP_Silk_decoder_state *psDec, SKP_int16 pOut[], SKP_int16 *pN, const SKP_uint8 pCode[], const SKP_int16 nBytes[],
                                     SKP_int action, SKP_int decBytes[]) {
    const SKP_int ret = __real_SKP_Silk_decode_frame(psDec, pOut, pN, pCode, nBytes, action, decBytes);
    const int L = 20 * solo_dec_tap_fs;
    if (psDec->frame_length == L && solo_dec_tap_lo_n + L <= (int)(sizeof(solo_dec_tap_lo) / sizeof(short))) memcpy(solo_dec_tap_lo + solo_dec_tap_lo_n, pOut, sizeof(short) * (size_t)L);
    solo_dec_tap_lo_n += L;
    return ret;
}

/* ---- high band ---- */
static int hb_sub = 0;
void __real_AGR_Sate_lsp_dequant_highband(SKP_int32 *, SKP_int32, SKP_int32);
void __wrap_AGR_Sate_lsp_dequant_highband(SKP_int32 *qlsp, SKP_int32 idx, SKP_int32 order) {
    __real_AGR_Sate_lsp_dequant_highband(qlsp, idx, order);
    if (solo_dec_tap_hb_n < DPK_MAX * 2) put(solo_dec_tap_hb[solo_dec_tap_hb_n], qlsp, 8, 4);
}
void __real_AGR_Sate_LPC_synthesis_filter_fix(const SKP_int32 *, const SKP_int16 *, const SKP_int32, SKP_int32 *, SKP_int16 *, const SKP_int32, const SKP_int);
void __wrap_AGR_Sate_LPC_synthesis_filter_fix(const SKP_int32 *in_Q10, const SKP_int16 *A_Q12, const SKP_int32 Gain_Q16, SKP_int32 *S, SKP_int16 *out,
                                              const SKP_int32 len, const SKP_int Order) {
    __real_AGR_Sate_LPC_synthesis_filter_fix(in_Q10, A_Q12, Gain_Q16, S, out, len, Order);
    if (solo_dec_tap_hb_n < DPK_MAX * 2) {
        int *h = solo_dec_tap_hb[solo_dec_tap_hb_n];
        put(h + 8, A_Q12, 8, 2);
        h[16 + hb_sub] = Gain_Q16 / -FOLDING_GAIN_FIX;          /* the gain argument is -FOLDING_GAIN_FIX * the sub-frame gain */
    }
    if (solo_dec_tap_hi_n + len <= (int)(sizeof(solo_dec_tap_hi) / sizeof(short))) memcpy(solo_dec_tap_hi + solo_dec_tap_hi_n, out, sizeof(short) * (size_t)len);
    solo_dec_tap_hi_n += len;
    if (++hb_sub == HB_SUBFR) { hb_sub = 0; solo_dec_tap_hb_n++; }
}
void __real_AGR_Sate_qmf_synth(const SKP_int16 *, const SKP_int16 *, const SKP_int16 *, SKP_int16 *, SKP_int32, SKP_int32, SKP_int16 *, SKP_int16 *, SKP_int8 *);
void __wrap_AGR_Sate_qmf_synth(const SKP_int16 *x1, const SKP_int16 *x2, const SKP_int16 *a, SKP_int16 *y, SKP_int32 N, SKP_int32 M, SKP_int16 *mem1,
                               SKP_int16 *mem2, SKP_int8 *stack) {
    if (solo_dec_tap_qmf_n < DPK_MAX && N / 2 <= 640) {
        memcpy(solo_dec_tap_qmf[solo_dec_tap_qmf_n][0], x1, sizeof(short) * (size_t)(N / 2));
        memcpy(solo_dec_tap_qmf[solo_dec_tap_qmf_n][1], x2, sizeof(short) * (size_t)(N / 2));
        solo_dec_tap_qmf_n++;
    }
    __real_AGR_Sate_qmf_synth(x1, x2, a, y, N, M, mem1, mem2, stack);
}

/* ---- the state after every call, in the order of SxDecState (solo_amd/csrc/solo_dec.h) ---- */
SKP_int32 __real_AGR_Sate_decode_process(SATEDecCtl *, NovaBits *, SKP_int16 *, void *, void *, SKP_int16 *, SKP_int32);
SKP_int32 __wrap_AGR_Sate_decode_process(SATEDecCtl *sateCtl, NovaBits *bits, SKP_int16 *vout, void *skdecCtrl, void *hbdecCtrl, SKP_int16 nBytes[], SKP_int32 lostflag) {
    const SKP_int32 ret = __real_AGR_Sate_decode_process(sateCtl, bits, vout, skdecCtrl, hbdecCtrl, nBytes, lostflag);
    const SKP_Silk_decoder_state *d = (const SKP_Silk_decoder_state *)sateCtl->stDec;
    const AGR_Sate_decoder_hb_state_FIX *hb = (const AGR_Sate_decoder_hb_state_FIX *)sateCtl->stHBDec;
    const AGR_Sate_HB_decoder_control_FIX *hc = &sateCtl->HBdecControl;
    const int lpc = solo_dec_tap_fs == 8 ? 10 : 16, L = 20 * solo_dec_tap_fs;
    int *p0, *p, k, i;
    if (solo_dec_tap_state_n >= DPK_MAX) return ret;
    p0 = p = solo_dec_tap_state[solo_dec_tap_state_n++];
    *p++ = ret;
    *p++ = d->fs_kHz == solo_dec_tap_fs;                        /* 0: the decoder still runs at its initial 24 kHz: no low-band state recorded */
    if (d->fs_kHz == solo_dec_tap_fs) {
        for (k = 0; k < 2; k++) {
            const SKP_Silk_md_decoder_state *m = &d->sMD[k];
            *p++ = m->LastGainIndex; p = put(p, m->prevNLSF_Q15, lpc, 4); *p++ = m->typeOffsetPrev; *p++ = m->prevDeltaGainIndex;
            *p++ = m->sRC.bufferLength; *p++ = m->sRC.bufferIx; *p++ = m->sRC.error; *p++ = (int)m->sRC.base_Q32; *p++ = (int)m->sRC.range_Q16;
            *p++ = 0; *p++ = 0;                                 /* rc_tail, rc_stale: the build's own */
        }
        *p++ = d->prev_inv_gain_Q16;
        p = put(p, d->sLTP_Q16, 2 * L, 4); p = put(p, d->sLPC_Q14, 16, 4); p = put(p, d->exc_Q10, L, 4); p = put(p, d->outBuf, 2 * L, 2);
        *p++ = d->lagPrev; *p++ = d->first_frame_after_reset; *p++ = d->nFramesDecoded; *p++ = d->moreInternalDecoderFrames; *p++ = d->FrameTermination;
        *p++ = d->vadFlag; *p++ = d->lossCnt; *p++ = d->prev_sigtype; *p++ = d->nBytesLeft[0];
        *p++ = 0;                                               /* started: the build's own */
        p = put(p, d->HPState, 2, 4);
        p = put(p, d->sCNG.CNG_exc_buf_Q10, L, 4); p = put(p, d->sCNG.CNG_smth_NLSF_Q15, lpc, 4); p = put(p, d->sCNG.CNG_synth_state, lpc, 4);
        *p++ = d->sCNG.CNG_smth_Gain_Q16; *p++ = d->sCNG.rand_seed; *p++ = d->sCNG.fs_kHz;
        *p++ = d->sPLC.pitchL_Q8; p = put(p, d->sPLC.LTPCoef_Q14, 5, 2); p = put(p, d->sPLC.prevLPC_Q12, lpc, 2);
        *p++ = d->sPLC.last_frame_lost; *p++ = d->sPLC.rand_seed; *p++ = d->sPLC.randScale_Q14; *p++ = d->sPLC.prevLTP_scale_Q14;
        *p++ = d->sPLC.conc_energy; *p++ = d->sPLC.conc_energy_shift; p = put(p, d->sPLC.prevGain_Q16, 4, 4); *p++ = d->sPLC.fs_kHz;
    } else {
        p += 2 * (lpc + 10) + 1 + 2 * L + 16 + L + 2 * L + 12 + L + 2 * lpc + 3 + 1 + 5 + lpc + 6 + 4 + 1;
    }
    *p++ = hb->hb_lossCnt; *p++ = hc->first;
    *p++ = 0; *p++ = 0;                                         /* hb_joint, fpp: the build's configuration */
    p = put(p, hb->HB_prev_NLSFq_fix, 8, 4); p = put(p, hb->HB_synth_state, 8, 4); *p++ = hb->HB_prev_Gain_fix;
    for (i = 0; i < 32; i++) *p++ = hc->g0_mem[2 * (31 - i) + 1];   /* mem[2 i + 1] = the sample i + 1 before the end (AGR_BWE_qmf.c:178) */
    for (i = 0; i < 32; i++) *p++ = hc->g1_mem[2 * (31 - i) + 1];
    solo_dec_tap_state_ints = (int)(p - p0);
    return ret;
}

/* Test infrastructure only: stage taps for the compiled reference encoder.
 *
 * Linked into oracle/_ref/libsolo_ref_fix_taps.so together with the UNMODIFIED reference sources, with
 * -Wl,--wrap=<stage function> for each analysis stage of SKP_Silk_encode_frame_FIX (encode_frame_FIX.c:100-143).
 * Every wrapper calls the real function and then appends a canonical int32 record of the encoder control block
 * to a global tap buffer that the tests read through ctypes and compare with the same record produced by the
 * host emulation of the kernel source (tests/emu).  Nothing here is part of the product. */
#include <string.h>
#include "SKP_Silk_main_FIX.h"

#define TAP_REC 1024
#define TAP_MAX 64
int solo_tap_n = 0;
int solo_tap_buf[TAP_MAX][TAP_REC];

static int *put(int *p, const void *src, int n, int elem) {
    int i;
    for (i = 0; i < n; i++) {
        if (elem == 4) *p++ = ((const int *)src)[i];
        else if (elem == 2) *p++ = ((const short *)src)[i];
        else *p++ = ((const signed char *)src)[i];
    }
    return p;
}

static void tap(int stage, SKP_Silk_encoder_state_FIX *psEnc, SKP_Silk_encoder_control_FIX *c, const short *xfw,
                const signed char *q, signed char **q_md, const int *r) {
    int *p, *p0;
    if (solo_tap_n >= TAP_MAX) return;
    p0 = p = solo_tap_buf[solo_tap_n++];
    memset(p, 0, sizeof(int) * TAP_REC);
    *p++ = stage;
    *p++ = c->sCmn.sigtype; *p++ = c->sCmn.QuantOffsetType; *p++ = c->sCmn.lagIndex; *p++ = c->sCmn.contourIndex;
    *p++ = c->sCmn.PERIndex;
    p = put(p, c->sCmn.LTPIndex, 4, 4);
    p = put(p, c->sCmn.NLSFIndices, 6, 4);
    *p++ = c->sCmn.NLSFInterpCoef_Q2;
    p = put(p, c->sCmn.GainsIndices, 4, 4);
    *p++ = c->sCmn.DeltaGainsIndices; *p++ = c->sCmn.Seed; *p++ = c->sCmn.LTP_scaleIndex;
    p = put(p, c->sCmn.pitchL, 4, 4);
    p = put(p, c->Gains_Q16, 4, 4);
    *p++ = c->DeltaGains_Q16;
    p = put(p, c->PredCoef_Q12[0], 10, 2);
    p = put(p, c->PredCoef_Q12[1], 10, 2);
    p = put(p, c->LTPCoef_Q14, 20, 2);
    *p++ = c->LTP_scale_Q14;
    p = put(p, c->AR1_Q13, 64, 2);
    p = put(p, c->AR2_Q13, 64, 2);
    p = put(p, c->LF_shp_Q14, 4, 4);
    p = put(p, c->GainsPre_Q14, 4, 4);
    p = put(p, c->HarmBoost_Q14, 4, 4);
    p = put(p, c->Tilt_Q14, 4, 4);
    p = put(p, c->HarmShapeGain_Q14, 4, 4);
    *p++ = c->Lambda_Q10; *p++ = c->input_quality_Q14; *p++ = c->coding_quality_Q14; *p++ = c->current_SNR_dB_Q7;
    *p++ = c->sparseness_Q8; *p++ = c->predGain_Q16; *p++ = c->LTPredCodGain_Q7;
    p = put(p, c->input_quality_bands_Q15, 4, 4);
    *p++ = c->input_tilt_Q15;
    p = put(p, c->ResNrg, 4, 4);
    p = put(p, c->ResNrgQ, 4, 4);
    *p++ = psEnc->speech_activity_Q8; *p++ = psEnc->LTPCorr_Q15;
    /* p0 + 256: signals */
    p = p0 + 256;
    if (xfw) put(p, xfw, 160, 2);
    p += 160;
    if (q) put(p, q, 160, 1);
    p += 160;
    if (q_md) { put(p, q_md[0], 160, 1); put(p + 160, q_md[1], 160, 1); }
    p += 320;
    if (r) put(p, r, 160, 4);
}

static SKP_Silk_encoder_state_FIX *cur_enc;
static const short *cur_xfw;

void __real_SKP_Silk_find_pitch_lags_FIX(SKP_Silk_encoder_state_FIX *, SKP_Silk_encoder_control_FIX *, SKP_int16 *, const SKP_int16 *);
void __wrap_SKP_Silk_find_pitch_lags_FIX(SKP_Silk_encoder_state_FIX *psEnc, SKP_Silk_encoder_control_FIX *c, SKP_int16 *res, const SKP_int16 *x) {
    cur_enc = psEnc;
    __real_SKP_Silk_find_pitch_lags_FIX(psEnc, c, res, x);
    tap(1, psEnc, c, x + 40, 0, 0, 0);          /* signal slot: the high-passed input frame */
}
void __real_SKP_Silk_noise_shape_analysis_FIX(SKP_Silk_encoder_state_FIX *, SKP_Silk_encoder_control_FIX *, const SKP_int16 *, const SKP_int16 *);
void __wrap_SKP_Silk_noise_shape_analysis_FIX(SKP_Silk_encoder_state_FIX *psEnc, SKP_Silk_encoder_control_FIX *c, const SKP_int16 *pr, const SKP_int16 *x) {
    __real_SKP_Silk_noise_shape_analysis_FIX(psEnc, c, pr, x);
    tap(2, psEnc, c, pr, 0, 0, 0);              /* signal slot: pitch residual of the frame */
}
void __real_SKP_Silk_prefilter_FIX(SKP_Silk_encoder_state_FIX *, const SKP_Silk_encoder_control_FIX *, SKP_int16 *, const SKP_int16 *);
void __wrap_SKP_Silk_prefilter_FIX(SKP_Silk_encoder_state_FIX *psEnc, const SKP_Silk_encoder_control_FIX *c, SKP_int16 *xw, const SKP_int16 *x) {
    __real_SKP_Silk_prefilter_FIX(psEnc, c, xw, x);
    cur_xfw = xw;
    tap(3, psEnc, (SKP_Silk_encoder_control_FIX *)c, xw, 0, 0, 0);
}
void __real_SKP_Silk_find_pred_coefs_FIX(SKP_Silk_encoder_state_FIX *, SKP_Silk_encoder_control_FIX *, const SKP_int16 *);
void __wrap_SKP_Silk_find_pred_coefs_FIX(SKP_Silk_encoder_state_FIX *psEnc, SKP_Silk_encoder_control_FIX *c, const SKP_int16 *res) {
    __real_SKP_Silk_find_pred_coefs_FIX(psEnc, c, res);
    tap(4, psEnc, c, cur_xfw, 0, 0, 0);
}
void __real_SKP_Silk_process_gains_FIX(SKP_Silk_encoder_state_FIX *, SKP_Silk_encoder_control_FIX *);
void __wrap_SKP_Silk_process_gains_FIX(SKP_Silk_encoder_state_FIX *psEnc, SKP_Silk_encoder_control_FIX *c) {
    __real_SKP_Silk_process_gains_FIX(psEnc, c);
    tap(5, psEnc, c, cur_xfw, 0, 0, 0);
}
/* ---- isolated stage checks (tests/test_nsq_taps.py, tests/test_enc_stages.py): the ARGUMENTS of every SKP_Silk_NSQ_del_dec call (SKP_Silk_NSQ_del_dec.c:925)
 * in the layout of the build's hand-over record SxNsqIn (solo_amd/csrc/solo_enc_state.h: 340 bytes + the prefiltered frame; 660 bytes at the 8 kHz
 * internal rate, 980 at 16 kHz), and its outputs {int32 Seed; int8 q[2][L]; int32 r[L]}.  The records are packed at the stride of the run's frame
 * length L, which the first call after solo_nsq_tap_n = 0 fixes. */
#define NSQ_TAP_MAX 512
#define NSQ_TAP_LMAX 320
struct nsq_tap_head {
    int sigtype, QuantOffsetType, NLSFInterpCoef_Q2, Seed, Lambda_Q10, LTP_scale_Q14, DeltaGains_Q16;
    int pitchL[4], Gains_Q16[4], LF_shp_Q14[4], Tilt_Q14[4], HarmShapeGain_Q14[4];
    short PredCoef_Q12[2][16];
    short LTPCoef_Q14[20];
    short AR2_Q13[64];
};                                  /* + short xfw[L] */
int solo_nsq_tap_n = 0;
static int nsq_tap_L = 160;
unsigned char solo_nsq_tap_in[NSQ_TAP_MAX * (sizeof(struct nsq_tap_head) + 2 * NSQ_TAP_LMAX)];
unsigned char solo_nsq_tap_out[NSQ_TAP_MAX * (4 + 2 * NSQ_TAP_LMAX + 4 * NSQ_TAP_LMAX)];
int solo_nsq_tap_sizeof_in(void) { return (int)sizeof(struct nsq_tap_head) + 2 * nsq_tap_L; }
int solo_nsq_tap_sizeof_out(void) { return 4 + 2 * nsq_tap_L + 4 * nsq_tap_L; }
static int nsq_tap_seed_in;         /* the seed the frame went into the quantiser with (the coder's record keeps it: SxFrameIdx::Seed) */
static void nsq_tap_before(SKP_Silk_encoder_state *psEncC, SKP_Silk_encoder_control *c, const SKP_int16 *x, int LSFInterpFactor_Q2,
                           const SKP_int16 *PredCoef_Q12, const SKP_int16 *LTPCoef_Q14, const SKP_int16 *AR2_Q13, const SKP_int *HarmShapeGain_Q14,
                           const SKP_int *Tilt_Q14, const SKP_int32 *LF_shp_Q14, const SKP_int32 *Gains_Q16, SKP_int32 DeltaGains_Q16, int Lambda_Q10,
                           int LTP_scale_Q14) {
    struct nsq_tap_head *t;
    nsq_tap_seed_in = c->Seed;
    if (solo_nsq_tap_n == 0 && psEncC->frame_length <= NSQ_TAP_LMAX) nsq_tap_L = psEncC->frame_length;
    if (solo_nsq_tap_n >= NSQ_TAP_MAX || psEncC->frame_length != nsq_tap_L) return;
    t = (struct nsq_tap_head *)(solo_nsq_tap_in + (size_t)solo_nsq_tap_n * solo_nsq_tap_sizeof_in());
    memset(t, 0, sizeof(*t));
    t->sigtype = c->sigtype; t->QuantOffsetType = c->QuantOffsetType; t->NLSFInterpCoef_Q2 = LSFInterpFactor_Q2; t->Seed = c->Seed;
    t->Lambda_Q10 = Lambda_Q10; t->LTP_scale_Q14 = LTP_scale_Q14; t->DeltaGains_Q16 = DeltaGains_Q16;
    memcpy(t->pitchL, c->pitchL, sizeof(t->pitchL));
    memcpy(t->Gains_Q16, Gains_Q16, sizeof(t->Gains_Q16));
    memcpy(t->LF_shp_Q14, LF_shp_Q14, sizeof(t->LF_shp_Q14));
    memcpy(t->Tilt_Q14, Tilt_Q14, sizeof(t->Tilt_Q14));
    memcpy(t->HarmShapeGain_Q14, HarmShapeGain_Q14, sizeof(t->HarmShapeGain_Q14));
    memcpy(t->PredCoef_Q12, PredCoef_Q12, sizeof(t->PredCoef_Q12));          /* SKP_int16 PredCoef_Q12[2][MAX_LPC_ORDER] */
    {   /* the entries beyond the LPC order are never read and may hold whatever the caller's stack held: zeroed, so the record is
         * a function of the input alone */
        int k, o;
        for (k = 0; k < 2; k++)
            for (o = psEncC->predictLPCOrder; o < 16; o++) t->PredCoef_Q12[k][o] = 0;
    }
    memcpy(t->LTPCoef_Q14, LTPCoef_Q14, sizeof(t->LTPCoef_Q14));
    memcpy(t->AR2_Q13, AR2_Q13, sizeof(t->AR2_Q13));
    memcpy(t + 1, x, 2 * (size_t)nsq_tap_L);
}
static void nsq_tap_after(SKP_Silk_encoder_state *psEncC, SKP_Silk_encoder_control *c, SKP_int8 **q_md, const SKP_int32 *r) {
    unsigned char *t;
    if (solo_nsq_tap_n >= NSQ_TAP_MAX || psEncC->frame_length != nsq_tap_L) return;
    t = solo_nsq_tap_out + (size_t)solo_nsq_tap_n++ * solo_nsq_tap_sizeof_out();
    memcpy(t, &c->Seed, 4);
    memcpy(t + 4, q_md[0], nsq_tap_L); memcpy(t + 4 + nsq_tap_L, q_md[1], nsq_tap_L);
    memcpy(t + 4 + 2 * nsq_tap_L, r, 4 * (size_t)nsq_tap_L);
}
void __real_SKP_Silk_NSQ_del_dec(SKP_Silk_encoder_state *, SKP_Silk_encoder_control *, SKP_Silk_nsq_state *, SKP_Silk_nsq_state *,
    const SKP_int16 *, SKP_int8 *, SKP_int8 **, SKP_int32 *, const SKP_int, const SKP_int16 *, const SKP_int16 *, const SKP_int16 *,
    const SKP_int *, const SKP_int *, const SKP_int32 *, const SKP_int32 *, const SKP_int32 *, const SKP_int32, const SKP_int, const SKP_int);
void __wrap_SKP_Silk_NSQ_del_dec(SKP_Silk_encoder_state *psEncC, SKP_Silk_encoder_control *psEncCtrlC, SKP_Silk_nsq_state *NSQ,
    SKP_Silk_nsq_state *NSQ_md, const SKP_int16 *x, SKP_int8 *q, SKP_int8 **q_md, SKP_int32 *r, const SKP_int LSFInterpFactor_Q2,
    const SKP_int16 *PredCoef_Q12, const SKP_int16 *LTPCoef_Q14, const SKP_int16 *AR2_Q13, const SKP_int *HarmShapeGain_Q14,
    const SKP_int *Tilt_Q14, const SKP_int32 *LF_shp_Q14, const SKP_int32 *Gains_Q16, const SKP_int32 *MDGains_Q16,
    const SKP_int32 DeltaGains_Q16, const SKP_int Lambda_Q10, const SKP_int LTP_scale_Q14) {
    nsq_tap_before(psEncC, psEncCtrlC, x, LSFInterpFactor_Q2, PredCoef_Q12, LTPCoef_Q14, AR2_Q13, HarmShapeGain_Q14, Tilt_Q14, LF_shp_Q14, Gains_Q16,
                   DeltaGains_Q16, Lambda_Q10, LTP_scale_Q14);
    __real_SKP_Silk_NSQ_del_dec(psEncC, psEncCtrlC, NSQ, NSQ_md, x, q, q_md, r, LSFInterpFactor_Q2, PredCoef_Q12, LTPCoef_Q14, AR2_Q13,
        HarmShapeGain_Q14, Tilt_Q14, LF_shp_Q14, Gains_Q16, MDGains_Q16, DeltaGains_Q16, Lambda_Q10, LTP_scale_Q14);
    nsq_tap_after(psEncC, psEncCtrlC, q_md, r);
    /* sCmn is the first member of the FIX control / state structs */
    tap(6, cur_enc, (SKP_Silk_encoder_control_FIX *)psEncCtrlC, x, q, q_md, r);
}

/* ---- the coding stage's inputs (tests/test_enc_stages.py) ----
 * The coded indices of every frame in the field order of the build's SxFrameIdx (solo_amd/csrc/solo_enc.h), taken where the centre description's
 * parameters are coded (SKP_Silk_encode_frame_FIX.c:185: after the VAD / DTX flags of lines 151-165 are set).  A record is 20 ints + one per stage
 * of the run's NLSF codebooks (6 at the 8 kHz internal rate, 10 at 16 kHz).  Seed is the one the quantiser was CALLED with. */
#define IDX_TAP_MAX 512
#define IDX_TAP_INTS 32
int solo_idx_tap_n = 0, solo_idx_tap_ints = 0;
int solo_idx_tap[IDX_TAP_MAX][IDX_TAP_INTS];
void __real_SKP_Silk_encode_parameters(SKP_Silk_encoder_state *, SKP_Silk_encoder_control *, SKP_Silk_range_coder_state *, const SKP_int, const SKP_int8 *);
void __wrap_SKP_Silk_encode_parameters(SKP_Silk_encoder_state *psEncC, SKP_Silk_encoder_control *c, SKP_Silk_range_coder_state *psRC, const SKP_int md_type,
                                       const SKP_int8 *q) {
    if (md_type == 0 && psRC == &psEncC->sRC && solo_idx_tap_n < IDX_TAP_MAX) {
        const int stages = psEncC->fs_kHz == 8 ? 6 : 10;
        int *p0 = solo_idx_tap[solo_idx_tap_n++], *p = p0;
        memset(p0, 0, sizeof(int) * IDX_TAP_INTS);
        *p++ = c->sigtype; *p++ = c->QuantOffsetType;
        p = put(p, c->GainsIndices, 4, 4); *p++ = c->DeltaGainsIndices;
        p = put(p, c->NLSFIndices, stages, 4); *p++ = c->NLSFInterpCoef_Q2;
        *p++ = c->lagIndex; *p++ = c->contourIndex;
        if (c->sigtype == SIG_TYPE_VOICED) { *p++ = c->PERIndex; p = put(p, c->LTPIndex, 4, 4); *p++ = c->LTP_scaleIndex; }
        else p += 6;                /* an unvoiced frame never assigns them (SKP_Silk_find_pred_coefs_FIX.c:93-109; the control block is an uninitialised
                                     * local, SKP_Silk_encode_frame_FIX.c:41) and its coder never reads them (SKP_Silk_encode_parameters.c): left zero */
        *p++ = nsq_tap_seed_in; *p++ = psEncC->vadFlag;
        *p++ = psEncC->inDTX; *p++ = 0;
        solo_idx_tap_ints = (int)(p - p0);
    }
    __real_SKP_Silk_encode_parameters(psEncC, c, psRC, md_type, q);
}
/* The high band that the QMF analysis (AGR_BWE_qmf.c:38, called once per packet: AGR_BWE_encode_frame_FIX.c:119) hands to the high-band encoder:
 * N / 2 samples per call, packed. */
#define HI_TAP_MAX (64 * 640)
int solo_hi_tap_n = 0;              /* samples recorded */
short solo_hi_tap[HI_TAP_MAX];
void __real_AGR_Sate_qmf_decomp(const SKP_int16 *, const SKP_int16 *, SKP_int16 *, SKP_int16 *, SKP_int32, SKP_int32, SKP_int16 *, SKP_int8 *);
void __wrap_AGR_Sate_qmf_decomp(const SKP_int16 *xx, const SKP_int16 *aa, SKP_int16 *y1, SKP_int16 *y2, SKP_int32 N, SKP_int32 M, SKP_int16 *mem, SKP_int8 *stack) {
    __real_AGR_Sate_qmf_decomp(xx, aa, y1, y2, N, M, mem, stack);
    if (solo_hi_tap_n + N / 2 <= HI_TAP_MAX) { memcpy(solo_hi_tap + solo_hi_tap_n, y2, sizeof(short) * (size_t)(N / 2)); solo_hi_tap_n += N / 2; }
}

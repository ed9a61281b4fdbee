// solo_fn_probe.h -- function-level probe of the LPC / NLSF stage functions (tests only): ONE case = one call of one stage function with
// the work structures, the template site and the literal arguments of the product's call site, from an int32 record and back into one.
// Used by the gfx950 build (solo_fn_probe.hip: one wavefront per case, solo_debug_fn) and by the host emulation (tests/emu: emu_fn); the
// record layouts are restated in tests/fn_probe_lib.py.  What it runs is the stage function's body AS COMPILED FOR THE PROBE'S CALL: the
// product kernels keep their own specialised copies, which only whole-encoder inputs reach.
//
// fn = 4 * unit + site.  L = SX_LPC of the build; every vector is padded to 16 words (unused words: 0 in, 0 out).
//   unit 0  a2nlsf         site 0 / 1: sx_a2nlsf<0 / 1>, order L (sx_find_LPC's two calls); site 2: sx_a2nlsf<2>, order SX_HB_LPC (high band)
//                          in  a_Q16[16]                                     out NLSF[16], a_Q16[16] after the call
//   unit 1  nlsf2a_stable  site 0: order L, site 2: order SX_HB_LPC -- the row form with the callers' fall-back to the serial form
//                          in  NLSF[16] (each in 0 .. 32767)                 out AR_Q12[16], declined (1: the row form handed the call to
//                                                                            the serial form, 0: it did not; -1: this build has no row form)
//   unit 2  msvq           site 0: sx_nlsf_msvq_encode
//                          in  NLSF[16], prev_q[16], W_Q6[16], sigtype (0 / 1), mu_Q15, mu_fluc_red_Q16, deactivate_fluc_red
//                                                                            out NLSFIndices[16], quantised NLSF[16]
//   unit 3  burg           site 0: sx_burg_modified<0> (4 x (SX_SUBFR + L), order L), site 1: <1> (the frame's second half: 2 blocks),
//                          site 2: <2> (4 x SX_HB_LPCBLK, order SX_HB_LPC)
//                          in  x[SX_FNP_X] (one sample per word)             out res_nrg, res_nrg_Q, A_Q16[16]
//   unit 4  find_lpc       site 0: sx_find_LPC
//                          in  x[SX_FNP_X], prev_NLSFq[16] (0 .. 32767), useInterp   out NLSF_Q15[16], interpIndex
// A record whose words lie outside what is stated above (they would index a table) is not run: every output word is SX_FNP_REFUSED.
#pragma once
#include "solo_enc.h"

#define SX_FNP_A2NLSF 0
#define SX_FNP_NLSF2A 1
#define SX_FNP_MSVQ 2
#define SX_FNP_BURG 3
#define SX_FNP_FIND_LPC 4
#define SX_FNP_UNITS 5
#define SX_FNP_REFUSED ((i32)0x80000001)
#define SX_FNP_XL (4 * (SX_SUBFR + SX_LPC))
#define SX_FNP_XH (4 * SX_HB_LPCBLK)
#define SX_FNP_X (SX_FNP_XL > SX_FNP_XH ? SX_FNP_XL : SX_FNP_XH)

// words of a case's input and output record; false: no such (unit, site)
SX_HD bool sx_fn_probe_words(int fn, int* in_words, int* out_words) {
    const int unit = fn >> 2, site = fn & 3;
    if (fn < 0) return false;
    switch (unit) {
    case SX_FNP_A2NLSF: if (site > 2) return false; *in_words = 16; *out_words = 32; return true;
    case SX_FNP_NLSF2A: if (site != 0 && site != 2) return false; *in_words = 16; *out_words = 17; return true;
    case SX_FNP_MSVQ: if (site != 0) return false; *in_words = 52; *out_words = 32; return true;
    case SX_FNP_BURG: if (site > 2) return false; *in_words = SX_FNP_X; *out_words = 18; return true;
    case SX_FNP_FIND_LPC: if (site != 0) return false; *in_words = SX_FNP_X + 17; *out_words = 17; return true;
    }
    return false;
}

struct SxFnProbeWork {                // LDS: the work structures of the prediction analysis and of the high-band encoder, as the product lays them out
    SxPredWork pred;
    SxMsvqAux aux;
    SxHbWork hb;
    i32 prev[SX_MAX_LPC], idx[16], interp;
};

// the serial form behind the row form, as the product's callers write it (solo_enc.h, sx_hb_encode_frame): -> the `declined` word
template <int ORDER>
SX_HD i32 sx_fn_probe_nlsf2a(i16* A_Q12, const i32* NLSF_Q15, i32* ws) {
    i32 declined = -1;
#if defined(SX_LANE_STREAM) && defined(SX_HAVE_ROW_NLSF2A)
    declined = __builtin_amdgcn_ballot_w64(!sx_row_nlsf2a_stable_n<ORDER>(A_Q12, NLSF_Q15)) != 0 ? 1 : 0;
    if (declined)
#endif
    {
        wv_sync();
        if (SX_LANE == 0) sx_nlsf2a_stable_ws(SX_VPTR(A_Q12), SX_VPTR(NLSF_Q15), ORDER, SX_VPTR(ws));
    }
    wv_sync();
    return declined;
}

// all of v[0 .. n) in 0 .. 32767 (every lane looks at every word: the answer is wave-uniform)
SX_HD bool sx_fn_probe_nlsf_range(const i32* v, int n) {
    bool ok = true;
    for (int i = 0; i < n; i++) ok = ok && v[i] >= 0 && v[i] <= 32767;
    return ok;
}

template <int UNIT>
SX_HD void sx_fn_probe_case(SxFnProbeWork* w, int site, const i32* in, i32* out) {
    site = SX_UNI(site);
    int in_words = 0, out_words = 0;
    (void)sx_fn_probe_words(4 * UNIT + site, &in_words, &out_words);
    SxLpcWork* lw = &w->pred.u.lpc;
    bool ok = true;
    if constexpr (UNIT == SX_FNP_NLSF2A) ok = sx_fn_probe_nlsf_range(in, 16);
    if constexpr (UNIT == SX_FNP_MSVQ) ok = in[48] == 0 || in[48] == 1;
    if constexpr (UNIT == SX_FNP_FIND_LPC) ok = sx_fn_probe_nlsf_range(in + SX_FNP_X, 16);
    if (!ok) {
        SX_PAR(i, out_words) out[i] = SX_FNP_REFUSED;
        return;
    }
    if constexpr (UNIT == SX_FNP_A2NLSF) {
        const int d = site == 2 ? SX_HB_LPC : SX_LPC;
        i32* a = site == 2 ? w->hb.lpc.a_Q16 : (site == 1 ? lw->a_tmp_Q16 : lw->a_Q16);
        i32* nl = site == 2 ? w->hb.NLSF_Q15 : w->pred.NLSF_Q15;
        SX_PAR(i, 16) { a[i] = i < d ? in[i] : 0; nl[i] = 0; }
        wv_sync();
        if (site == 0) sx_a2nlsf(nl, a, SX_LPC, lw->P, lw->Q, &lw->u.grid);
        else if (site == 1) sx_a2nlsf<1>(nl, a, SX_LPC, lw->P, lw->Q, &lw->u.grid);
        else sx_a2nlsf<2>(nl, a, SX_HB_LPC, w->hb.lpc.P, w->hb.lpc.Q, &w->hb.lpc.u.grid);
        wv_sync();
        SX_PAR(i, 16) { out[i] = i < d ? nl[i] : 0; out[16 + i] = i < d ? a[i] : 0; }
    }
    if constexpr (UNIT == SX_FNP_NLSF2A) {
        const int d = site == 2 ? SX_HB_LPC : SX_LPC;
        i32* nl = site == 2 ? w->hb.NLSF_Q15 : w->pred.NLSF_Q15;
        i16* A = site == 2 ? w->hb.A_Q12 : lw->a_tmp_Q12;
        SX_PAR(i, 16) { nl[i] = i < d ? in[i] : 0; A[i] = 0; }
        wv_sync();
        const i32 declined = site == 2 ? sx_fn_probe_nlsf2a<SX_HB_LPC>(A, nl, w->hb.ws) : sx_fn_probe_nlsf2a<SX_LPC>(A, nl, lw->u.it.ws[0]);
        SX_PAR(i, 16) out[i] = i < d ? (i32)A[i] : 0;
        if (SX_LANE == 0) out[16] = declined;
    }
    if constexpr (UNIT == SX_FNP_MSVQ) {
        SxMsvqWork* mw = &w->pred.u.msvq;
        SX_PAR(i, 16) {
            w->pred.NLSF_Q15[i] = i < SX_LPC ? in[i] : 0;
            w->prev[i] = i < SX_LPC ? in[16 + i] : 0;
            mw->W_Q6[i] = i < SX_LPC ? in[32 + i] : 0;
            w->idx[i] = 0;
        }
        wv_sync();
        sx_nlsf_msvq_encode(w->idx, w->pred.NLSF_Q15, SX_UNI(in[48]), w->prev, mw->W_Q6, SX_UNI(in[49]), SX_UNI(in[50]), SX_UNI(in[51]), mw, &w->aux);
        wv_sync();
        SX_PAR(i, 16) { out[i] = i < SX_NLSF_STAGES ? w->idx[i] : 0; out[16 + i] = i < SX_LPC ? w->pred.NLSF_Q15[i] : 0; }
    }
    if constexpr (UNIT == SX_FNP_BURG) {
        const int sl = SX_SUBFR + SX_LPC;
        i32 e = 0, q = 0;
        i32* a = site == 2 ? w->hb.lpc.a_Q16 : (site == 1 ? lw->a_tmp_Q16 : lw->a_Q16);
        SX_PAR(i, 16) a[i] = 0;
        if (site == 2) { SX_PAR(i, SX_FNP_XH) w->hb.lpc_in[i] = (i16)in[i]; }
        else if (site == 1) { SX_PAR(i, 2 * sl) w->pred.LPC_in_pre[2 * sl + i] = (i16)in[i]; }
        else { SX_PAR(i, SX_FNP_XL) w->pred.LPC_in_pre[i] = (i16)in[i]; }
        wv_sync();
        if (site == 0) sx_burg_modified(&e, &q, a, w->pred.LPC_in_pre, sl, 4, K_FIND_LPC_COND_FAC_Q32, SX_LPC, &lw->burg);
        else if (site == 1) sx_burg_modified<1>(&e, &q, a, w->pred.LPC_in_pre + 2 * sl, sl, 2, K_FIND_LPC_COND_FAC_Q32, SX_LPC, &lw->burg);
        else sx_burg_modified<2>(&e, &q, a, w->hb.lpc_in, SX_HB_LPCBLK, 4, K_FIND_LPC_COND_FAC_Q32, SX_HB_LPC, &w->hb.lpc.burg);
        wv_sync();
        const int d = site == 2 ? SX_HB_LPC : SX_LPC;
        if (SX_LANE == 0) { out[0] = e; out[1] = q; }
        SX_PAR(i, 16) out[2 + i] = i < d ? a[i] : 0;
    }
    if constexpr (UNIT == SX_FNP_FIND_LPC) {
        SX_PAR(i, SX_FNP_XL) w->pred.LPC_in_pre[i] = (i16)in[i];
        SX_PAR(i, 16) { w->prev[i] = i < SX_LPC ? in[SX_FNP_X + i] : 0; w->pred.NLSF_Q15[i] = 0; }
        if (SX_LANE == 0) w->interp = 0;
        wv_sync();
        sx_find_LPC(w->pred.NLSF_Q15, &w->interp, w->prev, SX_UNI(in[SX_FNP_X + 16]) == 1 ? 1 : 0, SX_LPC, w->pred.LPC_in_pre, SX_SUBFR + SX_LPC, w->pred.LPC_res, lw);
        wv_sync();
        SX_PAR(i, 16) out[i] = i < SX_LPC ? w->pred.NLSF_Q15[i] : 0;
        if (SX_LANE == 0) out[16] = w->interp;
    }
}

// Host emulation build of the KERNEL SOURCE (solo_amd/csrc/*.h) -- test infrastructure only.
//
// The codec kernels are written wave-uniform (solo_wave.h); compiled without hipcc the same source
// runs with SX_NLANES == 1, which lets the CPU-side tests (-m "not gpu") check the kernel source
// against the reference / golden vectors in a container that has no GPU.  Nothing in the product
// library (solo_amd/csrc/solo_api.hip) links or calls this file.
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
// -DSX_FS_KHZ=16 -DEMU_DEC_ONLY builds the 32 kHz-mode decoder (libsolo_emu_wb.so): same entry points, 1280-sample packets.
#ifndef EMU_DEC_ONLY
struct SxEncState; struct SxEncWork;
static void emu_tap(int stage, const SxEncState* st, const SxEncWork* w, const int16_t* sig);
#define SX_ENC_TAP(stage, st, w, sig) emu_tap(stage, st, w, sig)
#endif
#include "../../solo_amd/csrc/solo_dec.h"
#include "../../solo_amd/csrc/solo_l0_probe.h"
#include "../../solo_amd/csrc/solo_recv.h"
#ifndef EMU_DEC_ONLY
#include "../../solo_amd/csrc/solo_enc.h"
#include "../../solo_amd/csrc/solo_fn_probe.h"
#endif

extern "C" {

struct EmuDec { SxDecState st; SxDecWork w; SxDecShadow sh; int useMDIndex; SxExtractLane L; int two_step; };

void* emu_dec_create(int useMDIndex) {                    // bit 1 of the argument: joint_mode 1 (40 ms high-band frame), bit 3: framesize_ms 20
    EmuDec* d = (EmuDec*)calloc(1, sizeof(EmuDec));
    sx_dec_state_init(&d->st, ((useMDIndex >> 1) & 1) | (((useMDIndex >> 3) & 1) << 1));
    d->useMDIndex = useMDIndex & 1;
    return d;
}
void emu_dec_destroy(void* h) { free(h); }
// on: decode like the batch path's two kernels -- the packet's descriptions go through the history-free extraction step
// (sx_extract_desc) first, the decoder proper then continues from its records where they are usable
void emu_dec_set_split(void* h, int on) { ((EmuDec*)h)->two_step = on; }
static int emu_usable_count = 0, emu_fallback_count = 0;
int emu_dec_two_step_stats(int which) { return which ? emu_fallback_count : emu_usable_count; }
// the extraction step alone (tests/test_dec_stages.py): the records solo_dec_extract_kernel leaves for the two description slots of ONE packet
// handed over as (bits, nBytes0, nBytes1, lostflag); a slot without a description gets usable = 0 and nothing else (solo_dec_list_kernel).
// fill: what the records hold before (0: like solo_debug_dec_extract; 0xA5: whatever the decoder takes from a record must have been written)
void emu_dec_extract(void* h, const uint8_t* bits, int nBytes0, int nBytes1, int lostflag, void* recs2, int fill) {
    EmuDec* d = (EmuDec*)h;
    SxExtracted* ext2 = (SxExtracted*)recs2;
    sx_cdf_load_dec(&d->w.cdf);
    memset(ext2, fill, 2 * sizeof(SxExtracted));
    const int hb_joint = d->st.hb_joint | (d->st.fpp == 1);   // (solo_dec_extract_kernel: four high-band bytes instead of eight)
    for (int md = 0; md < 2; md++) {                      // one lane per description slot
        ext2[md].usable = 0;
        i32 off = 0, len = 0, hb_off = -1;
        int sel = 0;
        if (sx_desc_span(lostflag, nBytes0, nBytes1, hb_joint, md, &off, &len, &sel, &hb_off))
            sx_extract_desc(bits + off, len, d->useMDIndex, (const SxCdf*)&d->w.cdf, &d->L, &ext2[md], sel, hb_off >= 0 ? bits + hb_off : 0, hb_joint);
    }
}
// the decoder proper alone: recs2 = the packet's two records (emu_dec_extract's or the caller's own) or NULL (the decoder reads its symbols itself)
int emu_dec_packet_recs(void* h, const uint8_t* bits, int nBytes0, int nBytes1, int lostflag, const void* recs2, int16_t* pcm) {
    EmuDec* d = (EmuDec*)h;
    const SxExtracted* ext2 = (const SxExtracted*)recs2;
    sx_cdf_load_dec(&d->w.cdf);
    if (ext2 && lostflag >= 2) { if (sx_extracted_usable(&d->st, ext2, lostflag)) emu_usable_count++; else emu_fallback_count++; }
    d->w.st = d->st;                                      // the kernel keeps state + tables in LDS for a launch
    d->w.shadow = &d->sh;
    int r = sx_decode_packet(&d->w, bits, nBytes0, nBytes1, lostflag, d->useMDIndex, pcm, ext2);
    d->st = d->w.st;
    return r;
}
int emu_dec_packet(void* h, const uint8_t* bits, int nBytes0, int nBytes1, int lostflag, int16_t* pcm) {
    EmuDec* d = (EmuDec*)h;
    SxExtracted ext2[2];
    if (d->two_step) emu_dec_extract(h, bits, nBytes0, nBytes1, lostflag, ext2, 0xA5);
    return emu_dec_packet_recs(h, bits, nBytes0, nBytes1, lostflag, d->two_step ? ext2 : 0, pcm);
}
int emu_sizeof_extracted() { return (int)sizeof(SxExtracted); }
int emu_sizeof_frame_syms() { return (int)sizeof(SxFrameSyms); }
int emu_sizeof_dec_ctrl() { return (int)sizeof(SxDecCtrl); }
// L0 vocabulary, operand by operand (tests/test_l0_primitives.py)
void emu_l0(int op, int n, const int32_t* a, const int32_t* b, const int32_t* c, int32_t* out) {
    for (int i = 0; i < n; i++) out[i] = sx_l0_probe(op, a[i], b[i], c[i]);
}
void emu_sum_sqr_shift(const int16_t* x, int len, int odd_start, int32_t* energy, int32_t* shift) { sx_sum_sqr_shift(energy, shift, x, len, odd_start); }
int emu_sizeof_dec_state() { return (int)sizeof(SxDecState); }
int emu_sizeof_dec_work() { return (int)sizeof(SxDecWork); }
int emu_packet_samples() { return SX_PACKET; }

// receiver staging ring: the bookkeeping of solo_recv_insert_kernel (window check, slot claim), one arrival after the other
void emu_recv_file(const int32_t* arrivals, int n, int n_streams, int depth, int slot, const uint8_t* payload, long long payload_bytes, int useMDIndex,
                   const int32_t* play, uint32_t* lens, int32_t* verdict, int32_t* slot_out) {
    for (int a = 0; a < n; a++) {
        SxRecvArrival r = {arrivals[5 * a], arrivals[5 * a + 1], arrivals[5 * a + 2], arrivals[5 * a + 3], arrivals[5 * a + 4]};
        int sl = -1;
        int v = sx_recv_file(&r, payload, payload_bytes, n_streams, depth, slot, useMDIndex, play, lens, 1, &sl);
        if (v == SX_RECV_INSERTED && sl < 0) v = SX_RECV_DUP;
        verdict[a] = v; slot_out[a] = sl;
    }
}

}  // extern "C"

// debug aid: raw view of the decoder state (tests only)
extern "C" const void* emu_dec_state_ptr(void* h) { return &((EmuDec*)h)->st; }

#ifndef EMU_DEC_ONLY
// ---- encoder ----
extern "C" {
struct EmuEnc { SxEncStream rec; SxEncWork w; SxCodeIn cin; };
void* emu_enc_create(int rate_bps, int useMDIndex) {        // bit 1 of the second argument: joint_mode 1, bit 2: DTX, bit 3: framesize_ms 20
    EmuEnc* e = (EmuEnc*)calloc(1, sizeof(EmuEnc));
    const int joint = (useMDIndex >> 1) & 1;
    sx_enc_state_init(&e->rec, rate_bps - (joint ? 800 : 1600), useMDIndex & 1, joint, (useMDIndex >> 2) & 1, ((useMDIndex >> 3) & 1) ? 1 : 2);   // AGR_BWE_SDK_API.c:119
    return e;
}
void emu_enc_destroy(void* h) { free(h); }
int emu_enc_packet(void* h, const int16_t* pcm, uint8_t* bits, int buf_size, int16_t* nBytesOut) {
    EmuEnc* e = (EmuEnc*)h;
    e->w.st = e->rec.core;                                    // the kernel keeps the compact state in LDS for a launch
    int r = sx_encode_packet(&e->rec, &e->w, &e->cin, pcm, bits, buf_size, nBytesOut);
    e->rec.core = e->w.st;
    return r;
}
// the quantiser alone (tests/test_nsq_taps.py): n frames of ONE freshly initialised stream, in = SxNsqIn[n], out = SxNsqOut[n]
int emu_nsq_frames(const void* in, int n, void* out) {
    EmuEnc* e = (EmuEnc*)emu_enc_create(13600, 0);
    for (int f = 0; f < n; f++)
        sx_nsq_del_dec((char*)&e->rec.nsq, 0u, (const SxNsqIn*)in + f, (char*)((SxNsqOut*)out + f), 0u, &e->w.u.nsq, e->w.u.nsq.ring_emu, 0u, 12);
    emu_enc_destroy(e);
    return (int)sizeof(SxNsqOut);
}
// the analysis stage alone (tests/test_enc_stages.py): n_packets of ONE freshly initialised stream (arguments as emu_enc_create's) through
// sx_enc_stage_a -> in2 = SxNsqIn[n_packets][2], cin = SxCodeIn[n_packets].  chunk > 0: the compact state goes back to the stream record and
// is loaded again every `chunk` packets, as between two launches of solo_enc_analysis_kernel
int emu_analysis_packets(int rate_bps, int useMDIndex, const int16_t* pcm, int n_packets, int chunk, void* in2, void* cin) {
    EmuEnc* e = (EmuEnc*)emu_enc_create(rate_bps, useMDIndex);
    const int cp = chunk > 0 ? chunk : n_packets;
    for (int p0 = 0; p0 < n_packets; p0 += cp) {
        e->w.st = e->rec.core;
        for (int p = p0; p < p0 + cp && p < n_packets; p++)
            sx_enc_stage_a(&e->rec, &e->w, pcm + (size_t)p * (SX_FRAME * 2 * e->w.st.fpp), (SxNsqIn*)in2 + 2 * p, (SxCodeIn*)cin + p);
        e->rec.core = e->w.st;
    }
    emu_enc_destroy(e);
    return (int)sizeof(SxNsqIn);
}
// the coding stage alone: cin = SxCodeIn[n_packets], out2 = SxNsqOut[n_packets][2] -> bits[n_packets][slot_bytes], nbytes[n_packets][2]; returns the
// first negative status (0: none).  Like solo_enc_coding_kernel / solo_enc_rc_kernel it loads the compact state at the start of every chunk and
// never writes it back: of the stream record the stage owns the high-band history only
int emu_coding_packets(int rate_bps, int useMDIndex, const void* cin, const void* out2, int n_packets, int chunk, int slot_bytes, uint8_t* bits, int16_t* nbytes) {
    EmuEnc* e = (EmuEnc*)emu_enc_create(rate_bps, useMDIndex);
    const int cp = chunk > 0 ? chunk : n_packets;
    int status = 0;
    for (int p0 = 0; p0 < n_packets; p0 += cp) {
        e->w.st = e->rec.core;
        for (int p = p0; p < p0 + cp && p < n_packets; p++) {
            const int r = sx_enc_stage_c(&e->rec, &e->w, (const SxCodeIn*)cin + p, (const SxNsqOut*)out2 + 2 * p, bits + (size_t)p * slot_bytes, slot_bytes, nbytes + 2 * p);
            if (r < 0 && status == 0) status = r;
        }
    }
    emu_enc_destroy(e);
    return status;
}
int emu_sizeof_code_in() { return (int)sizeof(SxCodeIn); }
int emu_sizeof_nsq_out() { return (int)sizeof(SxNsqOut); }
// the pulse coder alone (tests/test_pulse_coder.py): one frame of pulses through a fresh range coder -> its bytes (SKP_Silk_encode_pulses.c:55)
int emu_encode_pulses(int sigtype, int QuantOffsetType, const int8_t* q, uint8_t* out, int* error) {
    static SxCdf cdf;
    sx_cdf_load(&cdf);
    alignas(4) u8 pw[SX_RC_PW_ROW];
    alignas(4) i8 qa[SX_FRAME + 4];
    memcpy(qa, q, SX_FRAME);
    static u8 buf[SX_RC_BUF_STRIDE];
    memset(buf, 0, sizeof(buf));
    SxRangeEnc rc;
    sx_rc_enc_init(&rc, buf);
    sx_encode_pulses(&rc, sigtype, QuantOffsetType, qa, &cdf, pw);
    i32 nb;
    sx_rc_length_bits(rc.bufferIx, rc.range_Q16, &nb);
    sx_rc_enc_wrap_up(&rc);
    if (nb > 0 && nb <= (i32)sizeof(buf)) memcpy(out, buf, (size_t)nb);
    *error = rc.error;
    return nb;
}
// ---- description writer (tests/test_dec_constructed.py, tests/golden/make_dec_constructed.py): codes CHOSEN symbols, so that the decoder's
// rarely taken branches get well-formed inputs.  A second statement of the bitstream layout next to sx_code_description: it shares the range
// encoder, the shell coder's split and the tables with the product and nothing else, and nothing under solo_amd/ calls it. ----
// the fewest LSB planes SKP_Silk_encode_pulses would give a block of 16 magnitudes of any width (combine_and_check, encode_pulses.c:86-110)
int emu_min_planes(const int32_t* q16) {
    const i32 maxp0 = T_max_pulses[0], maxp1 = T_max_pulses[1], maxp2 = T_max_pulses[2], maxp3 = T_max_pulses[3];
    for (int nrs = 0; nrs < 31; nrs++) {
        i32 c1[8], c2[4], c3[2];
        int bad = 0;
        for (int k = 0; k < 8; k++) { c1[k] = (abs(q16[2 * k]) >> nrs) + (abs(q16[2 * k + 1]) >> nrs); bad |= c1[k] > maxp0; }
        for (int k = 0; k < 4; k++) { c2[k] = c1[2 * k] + c1[2 * k + 1]; bad |= c2[k] > maxp1; }
        for (int k = 0; k < 2; k++) { c3[k] = c2[2 * k] + c2[2 * k + 1]; bad |= c3[k] > maxp2; }
        bad |= c3[0] + c3[1] > maxp3;
        if (!bad) return nrs;
    }
    return -1;
}
// pulses of one frame: q[SX_FRAME] of any width, planes[SX_FRAME / 16] = the LSB planes of every block as the CALLER chooses them (at least
// emu_min_planes of the block, or the shell coder has no code for it: returns -1), the rate level given
static int emu_write_pulses(SxRangeEnc* rc, int sigtype, int QuantOffsetType, int RateLevelIndex, const int32_t* q, const int32_t* planes, const SxCdf* cdf) {
    const int iter = SX_FRAME / 16;
    u8 top[SX_FRAME];                                        // the magnitudes without their LSB planes: what the shell coder codes
    i32 sum[SX_FRAME / 16];
    for (int i = 0; i < iter; i++) {
        if (planes[i] < emu_min_planes(&q[i * 16]) || planes[i] > 30) return -1;
        sum[i] = 0;
        for (int k = 0; k < 16; k++) { top[i * 16 + k] = (u8)(abs(q[i * 16 + k]) >> planes[i]); sum[i] += top[i * 16 + k]; }
    }
    sx_rc_enc(rc, RateLevelIndex, &cdf->cdf_rate_levels[sigtype * 10]);
    const u16* first = &cdf->cdf_pulses_per_block[RateLevelIndex * 21];
    const u16* more = &cdf->cdf_pulses_per_block[9 * 21];
    for (int i = 0; i < iter; i++) {
        const u16* t = first;
        for (int k = 0; k < planes[i]; k++) { sx_rc_enc(rc, 18 + 1, t); t = more; }
        sx_rc_enc(rc, sum[i], t);
    }
    for (int i = 0; i < iter; i++)
        if (sum[i] > 0) sx_shell_encoder(rc, &top[i * 16], 0, cdf);
    const u32 p_lsb = cdf->cdf_lsb[1];
    for (int i = 0; i < iter; i++)
        for (int k = 0; k < 16 && planes[i] > 0; k++)
            for (int j = planes[i] - 1; j >= 0; j--) sx_rc_enc_bin(rc, (abs(q[i * 16 + k]) >> j) & 1, p_lsb);
    const u32 p_sign = cdf->cdf_sign[sx_smulbb(10 - 1, (sigtype << 1) + QuantOffsetType) + RateLevelIndex];
    for (int i = 0; i < SX_FRAME; i++)
        if (q[i] != 0) sx_rc_enc_bin(rc, q[i] > 0, p_sign);
    return 0;
}
// ONE description of nframes (1..3) frames: syms = SxFrameSyms[nframes] (the symbols in coding order; fs_bad, NLSF_Q15 and the fields after
// vadFlag are not looked at), pulses[nframes][SX_FRAME], planes[nframes][SX_FRAME / 16], term[nframes] = the frame-termination symbol 0..3
// coded after each frame, whatever it is.  -> the number of bytes written to out (SKP_Silk_range_coder_get_length before the wrap-up, as the
// encoder counts them), or -1; *error = the range encoder's
int emu_write_desc(int nframes, int useMDIndex, const void* syms, const int32_t* pulses, const int32_t* planes, const int32_t* term, uint8_t* out, int cap, int* error) {
    static SxCdf cdf;
    sx_cdf_load(&cdf);
    static u8 buf[SX_RC_BUF_STRIDE];
    memset(buf, 0, sizeof(buf));
    *error = 0;
    if (nframes < 1 || nframes > 3) return -1;
    SxRangeEnc rc;
    sx_rc_enc_init(&rc, buf);
    int prev = 0;
    for (int f = 0; f < nframes; f++) {
        const SxFrameSyms* y = (const SxFrameSyms*)syms + f;
        const int sigtype = y->typeOffset >> 1, QuantOffsetType = y->typeOffset & 1;
        if (f == 0) {
            if (useMDIndex == 1) sx_rc_enc(&rc, y->MDIndex, cdf.cdf_mdindex);
            sx_rc_enc(&rc, SX_FS_KHZ == 8 ? 0 : 2, cdf.cdf_fs);
            sx_rc_enc(&rc, y->typeOffset, cdf.cdf_type_offset);
            sx_rc_enc(&rc, y->GainsIndices[0], &cdf.cdf_gain[sigtype * 65]);
        } else {
            sx_rc_enc(&rc, y->typeOffset, &cdf.cdf_type_offset_joint[prev * 5]);
            sx_rc_enc(&rc, y->GainsIndices[0], cdf.cdf_delta_gain);
        }
        prev = y->typeOffset;
        for (int i = 1; i < SX_NB_SUBFR; i++) sx_rc_enc(&rc, y->GainsIndices[i], cdf.cdf_delta_gain);
        if (f == 0) sx_rc_enc(&rc, y->DeltaGainIndices, cdf.cdf_md_delta_gain);
        {
            const i32 nvec0[SX_NLSF_STAGES] = T_NLSF_CB0_NVEC, nvec1[SX_NLSF_STAGES] = T_NLSF_CB1_NVEC;
            const u16* ncdf = sigtype == 0 ? cdf.nlsf_cb0_cdf : cdf.nlsf_cb1_cdf;
            int off = 0;
            for (int s = 0; s < SX_NLSF_STAGES; s++) {
                sx_rc_enc(&rc, y->NLSFIndices[s], ncdf + off);
                off += (sigtype == 0 ? nvec0[s] : nvec1[s]) + 1;
            }
        }
        sx_rc_enc(&rc, y->NLSFInterpCoef_Q2, cdf.cdf_nlsf_interp);
        if (sigtype == 0) {
            sx_rc_enc(&rc, y->lagIx, cdf.cdf_pitch_lag);
            sx_rc_enc(&rc, y->conIx, cdf.cdf_pitch_contour);
            sx_rc_enc(&rc, y->PERIndex, cdf.cdf_ltp_per);
            const u16* gcdf = y->PERIndex == 0 ? cdf.cdf_ltp_gain0 : (y->PERIndex == 1 ? cdf.cdf_ltp_gain1 : cdf.cdf_ltp_gain2);
            for (int k = 0; k < SX_NB_SUBFR; k++) sx_rc_enc(&rc, y->LTPIx[k], gcdf);
            sx_rc_enc(&rc, y->LTPscaleIx, cdf.cdf_ltpscale);
        }
        sx_rc_enc(&rc, y->Seed, cdf.cdf_seed);
        if (emu_write_pulses(&rc, sigtype, QuantOffsetType, y->RateLevelIndex, pulses + f * SX_FRAME, planes + f * (SX_FRAME / 16), &cdf) < 0) return -1;
        sx_rc_enc(&rc, y->vadFlag, cdf.cdf_vadflag);
        if (term[f] < 0 || term[f] > 3) return -1;
        sx_rc_enc(&rc, term[f], cdf.cdf_frame_term);
    }
    i32 nb;
    sx_rc_length_bits(rc.bufferIx, rc.range_Q16, &nb);
    sx_rc_enc_wrap_up(&rc);
    *error = rc.error;
    if (rc.error || nb <= 0 || nb > cap || nb > (i32)sizeof(buf)) return -1;
    memcpy(out, buf, (size_t)nb);
    return nb;
}
// the function-level probe of the LPC / NLSF stage functions (solo_amd/csrc/solo_fn_probe.h; tests/test_fn_probe_reference.py): the host twin
// of solo_debug_fn over the same records, one call of the stage function per case.  -> 0, -1: no such fn / not the fn's record sizes
int emu_fn(int fn, int n_cases, const int32_t* in, int in_words, int32_t* out, int out_words) {
    int iw = 0, ow = 0;
    if (!sx_fn_probe_words(fn, &iw, &ow) || iw != in_words || ow != out_words || n_cases < 0) return -1;
    static SxFnProbeWork w;
    for (int c = 0; c < n_cases; c++) {
        memset(&w, 0, sizeof(w));
        const int32_t* ic = in + (size_t)c * iw;
        int32_t* oc = out + (size_t)c * ow;
        switch (fn >> 2) {
        case SX_FNP_A2NLSF: sx_fn_probe_case<SX_FNP_A2NLSF>(&w, fn & 3, ic, oc); break;
        case SX_FNP_NLSF2A: sx_fn_probe_case<SX_FNP_NLSF2A>(&w, fn & 3, ic, oc); break;
        case SX_FNP_MSVQ: sx_fn_probe_case<SX_FNP_MSVQ>(&w, fn & 3, ic, oc); break;
        case SX_FNP_BURG: sx_fn_probe_case<SX_FNP_BURG>(&w, fn & 3, ic, oc); break;
        default: sx_fn_probe_case<SX_FNP_FIND_LPC>(&w, fn & 3, ic, oc); break;
        }
    }
    return 0;
}
int emu_fn_x_words() { return SX_FNP_X; }
int emu_frame_samples() { return SX_FRAME; }
int emu_sizeof_nsq_in() { return (int)sizeof(SxNsqIn); }
int emu_sizeof_enc_state() { return (int)sizeof(SxEncStream); }
int emu_sizeof_enc_work() { return (int)sizeof(SxEncWork); }
// debug taps (tests only): last frame's control block, pulses and residual
const void* emu_enc_ctrl_ptr(void* h) { return &((EmuEnc*)h)->w.ctrl; }
int emu_sizeof_enc_ctrl() { return (int)sizeof(SxEncCtrl); }
const void* emu_enc_q_ptr(void* h) { return &((EmuEnc*)h)->rec.nsq_out[0].q[0][0]; }
const void* emu_enc_idx_ptr(void* h) { return &((EmuEnc*)h)->cin.idx[0]; }
const void* emu_enc_state_ptr(void* h) { return &((EmuEnc*)h)->rec; }
}

// ---- stage taps: same canonical record as oracle/ref_taps.c ----
#define TAP_REC 1024
#define TAP_MAX 64
extern "C" { int solo_tap_n = 0; int solo_tap_buf[TAP_MAX][TAP_REC]; }
template <typename T> static int* tput(int* p, const T* src, int n) { for (int i = 0; i < n; i++) *p++ = (int)src[i]; return p; }
static void emu_tap(int stage, const SxEncState* st, const SxEncWork* w, const int16_t* sig) {
    if (solo_tap_n >= TAP_MAX) return;
    const SxEncCtrl* c = &w->ctrl;
    const int frame = stage >> 4;
    stage &= 15;
    int* p0 = solo_tap_buf[solo_tap_n++];
    int* p = p0;
    memset(p, 0, sizeof(int) * TAP_REC);
    *p++ = stage;
    *p++ = c->sigtype; *p++ = c->QuantOffsetType; *p++ = c->lagIndex; *p++ = c->contourIndex; *p++ = c->PERIndex;
    p = tput(p, c->LTPIndex, 4); p = tput(p, c->NLSFIndices, 6); *p++ = c->NLSFInterpCoef_Q2;
    p = tput(p, c->GainsIndices, 4); *p++ = c->DeltaGainsIndices; *p++ = c->Seed; *p++ = c->LTP_scaleIndex;
    p = tput(p, c->pitchL, 4); p = tput(p, c->Gains_Q16, 4); *p++ = c->DeltaGains_Q16;
    p = tput(p, c->PredCoef_Q12[0], 10); p = tput(p, c->PredCoef_Q12[1], 10); p = tput(p, c->LTPCoef_Q14, 20);
    *p++ = c->LTP_scale_Q14;
    p = tput(p, c->AR1_Q13, 64); p = tput(p, c->AR2_Q13, 64); p = tput(p, c->LF_shp_Q14, 4); p = tput(p, c->GainsPre_Q14, 4);
    p = tput(p, c->HarmBoost_Q14, 4); p = tput(p, c->Tilt_Q14, 4); p = tput(p, c->HarmShapeGain_Q14, 4);
    *p++ = c->Lambda_Q10; *p++ = c->input_quality_Q14; *p++ = c->coding_quality_Q14; *p++ = c->current_SNR_dB_Q7;
    *p++ = c->sparseness_Q8; *p++ = c->predGain_Q16; *p++ = c->LTPredCodGain_Q7;
    p = tput(p, c->input_quality_bands_Q15, 4); *p++ = c->input_tilt_Q15;
    p = tput(p, c->ResNrg, 4); p = tput(p, c->ResNrgQ, 4);
    *p++ = st->speech_activity_Q8; *p++ = st->LTPCorr_Q15;
    p = p0 + 256;
    if (sig) tput(p, sig, 160);
    p += 160;
    if (stage == 6) {
        p += 160;                                   // centre pulses are not kept by the kernel source
        p += 320 + 160;                             // pulses / excitation now live in the stream's HBM record, see test hooks
    }
}

#endif  // EMU_DEC_ONLY

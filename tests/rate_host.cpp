// Host build of the rate control stage (solo_amd/csrc/solo_rate.h) for tests/test_rate_model.py and tests/test_rate_abi.py, which compile
// this file into a temporary directory through tests/host_build.py.
#include <stddef.h>
#include <string.h>
#include "../solo_amd/csrc/solo_rate.h"

extern "C" {

int emu_rate_state_bytes() { return SX_RATE_STATE_WORDS * 4; }
int emu_rate_count_size() { return (int)sizeof(SxRateCount); }
int emu_rate_params_size() { return (int)sizeof(SxRateParams); }
int emu_rate_apply_count_size() { return (int)sizeof(SxRateApplyCount); }
int emu_rate_feedback_size() { return (int)sizeof(solo_rtcp_feedback_t); }

// the record the create and reset calls leave: 16 words
void emu_rate_init(int* state, int n_rows) {
    for (int r = 0; r < n_rows; r++)
        for (int w = 0; w < SX_RATE_STATE_WORDS; w++) state[r * SX_RATE_STATE_WORDS + w] = sx_rate_init_word(w);
}

// the host's checks of the three calls -> 1 = accepted
int emu_rate_params_ok(const int* params) { return sx_rate_params_ok((const SxRateParams*)params) ? 1 : 0; }
int emu_rate_update_call_ok(int n_rows, const void* feedback, const int* params, const void* target, const void* mode, const void* count) {
    return sx_rate_update_call_ok(n_rows, feedback, (const SxRateParams*)params, target, mode, count) ? 1 : 0;
}
int emu_rate_apply_call_ok(int n_streams, int have_enc, const void* streams, int n, const void* target, const void* count) {
    return sx_rate_apply_call_ok(n_streams, have_enc != 0, streams, n, target, count) ? 1 : 0;
}
int emu_rate_mask_call_ok(const void* mode, int n_rows, const void* streams, int n, int n_packets, const void* seq_base, const void* send) {
    return sx_rate_mask_call_ok(mode, n_rows, streams, n, n_packets, seq_base, send) ? 1 : 0;
}

// state: int32 [n_rows][16], carried by the caller.  -> 0, -1 = refused by the host's checks
int emu_rate_update(int n_rows, int* state, const unsigned* feedback, const int* params, int* target, unsigned char* mode, int* count) {
    if (!sx_rate_update_call_ok(n_rows, feedback, (const SxRateParams*)params, target, mode, count)) return -1;
    SxRateArgs a;
    a.feedback = feedback; a.state = state; a.target = target; a.mode = mode; a.count = count; a.p = *(const SxRateParams*)params; a.n_rows = n_rows;
    sx_rate_update_host(a);
    return 0;
}
// -> 0, -1 = refused by the host's checks, -2 = the list was refused (nothing written)
int emu_rate_send_mask(const unsigned char* mode, int n_rows, const int* streams, int n, int n_packets, const int* seq_base, int first_seq,
                       const unsigned char* send_in, unsigned char* send) {
    if (!sx_rate_mask_call_ok(mode, n_rows, streams, n, n_packets, seq_base, send)) return -1;
    SxRateMaskArgs a;
    a.mode = mode; a.map = streams; a.seq_base = seq_base; a.send_in = send_in; a.send = send;
    a.n_rows = n_rows; a.n = n; a.n_packets = n_packets; a.first_seq = first_seq;
    return sx_rate_send_mask_host(a) ? 0 : -2;
}

// one value of solo_batch_update_rates on an encoder state the caller brings as bytes (emu_rate_enc_state_bytes of them) -> SX_RATE_KEPT /
// _APPLIED / _REFUSED; and what solo_batch_update_streams does with a SILK rate on the same bytes, to compare with
int emu_rate_enc_state_bytes() { return (int)sizeof(SxEncState); }
int emu_rate_snr_offset(int which) { return (int)(which ? offsetof(SxEncState, SNRPerMD_dB_Q7) : offsetof(SxEncState, SNR_dB_Q7)); }
int emu_rate_apply_target(void* enc_state, int target_bps, int hb_joint, int min_silk_bps) {
    return sx_enc_apply_target((SxEncState*)enc_state, target_bps, hb_joint, min_silk_bps);
}
void emu_rate_setup_rate(void* enc_state, int silk_rate_bps) { sx_enc_setup_rate((SxEncState*)enc_state, silk_rate_bps); }

}

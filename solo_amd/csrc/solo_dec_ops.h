// solo_dec_ops.h -- what the host-side pipeline (solo_api.hip) needs of one build of the decoder kernels (solo_dec_kernels.h as
// compiled in solo_api.hip: 16 kHz API rate, in solo_api_wb.hip: 32 kHz): record sizes and launchers, like solo_enc_ops.h for the encoder.
// A handle holds the table of its rate (solo_batch::dops) and never asks which rate that is.
//
// Not in the table: solo_recv_launch_reset / solo_recv_launch_reset_list.  They write length words and play-out positions only, the same
// kernels at either rate, so solo_api.hip calls its own build's directly: the table lists what differs between the builds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "solo_stream_ctl.h"
#ifndef SOLO_DEC_OPS_DEFINED
#define SOLO_DEC_OPS_DEFINED
struct solo_dec_ops {
    size_t state_bytes;              // sizeof SxDecStream
    size_t extracted_bytes;          // extraction records per packet: two SxExtracted, two entries of the list of slots that carry bytes
    int packet_samples;              // 40 ms at the API rate
    // (the decoder's useMDIndex is per stream: SxDecStream::useMDIndex, written by the init kernels; no decode launch takes it)
    hipError_t (*init)(void* states, int n_streams, int hb_joint, int useMDIndex, hipStream_t s);
    // the listed streams only (solo_batch_reset_streams): records (stream, useMDIndex), validated by the caller
    hipError_t (*init_list)(void* states, const SxStreamCtl* recs, int n, int hb_joint, hipStream_t s);
    // the listed RUNNING streams (solo_batch_update_streams): same records; useMDIndex changes, nothing else of the state
    hipError_t (*ctl_list)(void* states, const SxStreamCtl* recs, int n, hipStream_t s);
    // (map, verdict: a subset call's stream list and verdict word, solo_stream_ctl.h; NULL, NULL: every stream of the handle)
    // single kernel: one wavefront per stream parses and synthesises
    hipError_t (*decode)(void* states, const uint8_t* bits, const int16_t* nbytes, const uint8_t* recv, int n_streams, int n_packets, int slot,
                         int16_t* pcm, int32_t* status, const int32_t* map, const uint32_t* verdict, hipStream_t s);
    // two kernels: packets [p0, p0 + pc) of every stream; recs: extracted_bytes x n_streams x pc bytes + 256
    hipError_t (*extract)(const void* states, const uint8_t* bits, const int16_t* nbytes, const uint8_t* recv, int n_streams, int n_packets, int p0,
                          int pc, int slot, void* recs, const int32_t* map, const uint32_t* verdict, hipStream_t s);
    hipError_t (*synth)(void* states, const uint8_t* bits, const int16_t* nbytes, const uint8_t* recv, int n_streams, int n_packets, int p0, int pc,
                        int slot, const void* recs, int16_t* pcm, int32_t* status, const int32_t* map, const uint32_t* verdict, hipStream_t s);
    // descriptions that arrive apart (solo_batch_decode_split)
    hipError_t (*split)(void* states, const uint8_t* descA, const int16_t* lenA, const uint8_t* descB, const int16_t* lenB, int n_streams,
                        int n_packets, int slot, int16_t* pcm, int32_t* status, hipStream_t s);
    // play-out from the receiver staging ring (solo_recv.h)
    hipError_t (*ring)(void* states, const uint8_t* ring, uint32_t* lens, int32_t* play, int n_streams, int n_packets, int depth, int slot,
                       int16_t* pcm, int32_t* status, const int32_t* map, const uint32_t* verdict, hipStream_t s);
    // one packet with the reference's raw (ptr, nBytes, lostflag) convention (AGR_Sate_Decoder_Decode)
    hipError_t (*raw)(void* state, const uint8_t* bits, int n0, int n1, int lostflag, int16_t* pcm, int32_t* status, hipStream_t s);
    // arrivals into the staging ring (reads each stream's useMDIndex from its decoder state); trk: the per-stream counters of
    // solo_recv_track (solo_recv.h), NULL = not counted
    hipError_t (*recv_insert)(const void* arrivals, int n_arr, const uint8_t* payload, long long payload_bytes, int n_streams, int depth, int slot,
                              const void* states, uint8_t* ring, uint32_t* lens, const int32_t* play, uint32_t* stats, uint32_t* trk, hipStream_t s);
};
#endif

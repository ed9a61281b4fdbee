/* solo_mi355x.h -- C ABI of libsolo_mi355x.so, the MI355X-native drop-in for the SOLO hot path.
 *
 * Part 1 re-declares, unchanged, the six entry points of the reference's public header
 *   JC1_SDK_SRC_ARM/interface/AGR_JC1_SDK_API.h:11-64   (identical in JC1_SDK_SRC_FLP/interface/)
 * so the reference's own callers (test/enc_main.c:190-274, test/dec_main.c:188-392, or a media
 * engine) link against this library instead of libJC1Codec.a without source changes.  Each handle is
 * a batch of ONE stream whose codec state lives in HBM; every call launches the same gfx950 kernels
 * as the batched API (there is no host-side codec arithmetic and no CPU fallback: if no HIP device is
 * usable, Init returns NULL and Encode/Decode return -1).
 * THESE SIX SYMBOLS ARE A CONFORMANCE AND MIGRATION PATH, NOT A REPLACEMENT FOR THE REFERENCE'S PER-CALL SPEED: a call is the
 * single-wavefront kernel chain of one packet end to end plus two small copies and one synchronisation -- Encode 1.06 ms (2.7 x the
 * reference's 0.39 ms on one host core), Decode 0.21 ms (8.8 x its 0.024 ms); tools/legacy_api_cost.py measures both.  One stream is
 * 1 / 4096 of what the device does in that time: throughput comes from Part 2.
 *
 * Part 2 is the additive batched API: N independent streams per handle, device pointers in,
 * device pointers out, one wavefront per stream.  This is what a server-side integration binds
 * (see INTEGRATION.md for the ctypes / cgo style stubs).
 */
#ifndef SOLO_MI355X_H
#define SOLO_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Part 1: reference-compatible surface (types from interface/SKP_Silk_typedef.h: SKP_int16=short,
 * SKP_int32=int, SKP_uint8=unsigned char)
 * ---------------------------------------------------------------------------------------------- */
typedef struct {            /* AGR_JC1_SDK_API.h:11-21 */
    int32_t mode;           /* ignored by the library (as in the reference)            */
    int32_t targetRate_bps; /* <=0 -> 15600 (AGR_BWE_SDK_API.c:35-37); CLI default 13600 */
    int32_t samplerate;     /* 16000, or 32000 (1280-sample packets, SILK wide band; targetRate_bps >= 15600) */
    int32_t dtx_enable;     /* 0 / 1                                                    */
    int32_t framesize_ms;   /* 40, or 20 (one SILK frame + one 4-byte high-band frame per packet: half the samples; not with joint_mode 1) */
    int32_t joint_enable;   /* 0, or 1 with joint_mode 1 (one 40 ms high-band frame)   */
    int32_t joint_mode;
    int32_t useMDIndex;     /* 0/1: one extra description-index symbol per description  */
} USER_Ctrl_enc;

typedef struct {            /* AGR_JC1_SDK_API.h:23-31 */
    int32_t packetLoss_perc;
    int32_t samplerate;     /* 16000, or 32000 (1280-sample packets, SILK wide band at 16 kHz) */
    int32_t framesize_ms;   /* 40 or 20, like the encoder's */
    int32_t joint_enable;
    int32_t joint_mode;
    int32_t useMDIndex;
} USER_Ctrl_dec;

/* AGR_JC1_SDK_API.h:33  (impl. libBWE/AGR_BWE_SDK_API.c:11).  NULL if the configuration is not the
 * supported one (samplerate 16000 or 32000, framesize 40 or 20, joint off or joint_mode 1 with framesize 40) or no GPU is available. */
void *AGR_Sate_Encoder_Init(USER_Ctrl_enc *enc_Ctrl);
/* AGR_JC1_SDK_API.h:37  (impl. AGR_BWE_SDK_API.c:129).  pcm: 640 samples (1280 at 32 kHz; half of that with framesize_ms 20); returns total bytes,
 * nBytesOut[0] = total, nBytesOut[1] = len(MD2)+8 (+4 with framesize_ms 20 or joint_mode 1) (MD1 = first nBytesOut[0]-nBytesOut[1] bytes). */
int32_t AGR_Sate_Encoder_Encode(void *SATEEnc_State, const int16_t *AGR_Sate_PCM, uint8_t *AGR_Sate_Bit,
                                int32_t AGR_Sate_Buf_Size, int16_t *nBytesOut);
/* AGR_JC1_SDK_API.h:45 */
int AGR_Sate_Encoder_Uninit(void *SATEEnc_State);
/* AGR_JC1_SDK_API.h:49  (impl. AGR_BWE_SDK_API.c:166) */
void *AGR_Sate_Decoder_Init(USER_Ctrl_dec *dec_Ctrl);
/* AGR_JC1_SDK_API.h:53  (impl. AGR_BWE_SDK_API.c:249).  lostflag: 1 lost, 2 MD1 only, 3 MD2(+HB) only,
 * 4 both.  Like the reference: -1 for nBytes[0] <= 0 with nothing touched; otherwise nBytes[0..1] are overwritten with the
 * low-band description lengths and *nSamplesOut is always written.  Unlike the reference, lengths that do not fit the buffer
 * contract (nBytes[0] > 1088, nBytes[1] outside [0, nBytes[0]], a second description shorter than its high-band bytes) are
 * refused with SKP_SILK_DEC_PAYLOAD_TOO_LARGE (-11) / SKP_SILK_DEC_PAYLOAD_ERROR (-12) instead of read out of bounds; on a
 * decoder error the PCM buffer is left untouched. */
int32_t AGR_Sate_Decoder_Decode(void *SATEDec_State, int16_t *AGR_Sate_PCM, int16_t *nSamplesOut,
                                const uint8_t *AGR_Sate_Bit, int16_t nBytes[], int32_t lostflag);
/* AGR_JC1_SDK_API.h:62 */
int32_t AGR_Sate_Decoder_Uninit(void *SATEDec_State);

/* ------------------------------------------------------------------------------------------------
 * Part 2: batched device API.  All d_* pointers are DEVICE pointers (HBM) of the current HIP device.
 *
 *   d_pcm      int16  [n_streams][n_packets][640]      stream-major 16 kHz PCM (1280 samples per packet at 32 kHz; half as many with framesize_ms 20)
 *   d_bits     uint8  [n_streams][n_packets][slot]     one fixed-size slot per packet: MD1|MD2|HB
 *   d_nbytes   int16  [n_streams][n_packets][2]        {total, len(MD2)+8}  (the reference's nBytesOut[0..1])
 *   d_recv     uint8  [n_streams][n_packets]           bit0: MD1 arrived, bit1: MD2(+HB) arrived
 *                                                      (3 -> lostflag 4, 1 -> 2, 2 -> 3, 0 -> 1; the
 *                                                       pointer/length mapping of test/dec_main.c:255-378
 *                                                       is done on the device)
 *   d_status   int32  [n_streams]                      0, or the first negative SILK error of the call
 *
 * Length records are validated on the device (0 <= len(MD2)+HB <= total <= slot): a record that violates this is never
 * dereferenced, the packet is concealed as lost and d_status reports -11 / -12.  DELIBERATE CONVENTION (not reference
 * behaviour): an empty record (total <= 0, e.g. a DTX packet that was not sent) is concealed as a lost packet (lostflag 1);
 * the reference library returns -1 for it without touching its state (AGR_BWE_SDK_API.c:266) and its CLI repeats the previous
 * output buffer -- the legacy AGR_Sate_Decoder_Decode symbol above keeps that behaviour.
 *
 * Streams keep their codec state in HBM inside the handle between calls (a call with n_packets = P
 * is identical to P calls with n_packets = 1).  Work is enqueued on `hip_stream` (a hipStream_t, may
 * be NULL for the default stream) and is asynchronous; no host synchronisation is performed.
 * Return value: 0 or a negative hipError_t.  solo_batch_encode returns -1 for n_packets >= ~700 000 (16 kHz) / ~350 000 (32 kHz) per
 * call -- split longer (offline) inputs over several calls; state carries over.
 * Device memory a handle holds besides the stream states: encode -- the hand-over records of one call, 4.3 KB per packet of the call
 * (n_streams x n_packets), and 32 KB of quantiser ring per four streams; decode -- one buffer of extraction records, 2216 B per
 * packet of a CHUNK (16 kHz API rate; 2 x sizeof(SxExtracted) + two entries of the list of slots that carry bytes: solo_api.hip asserts the figure): a call is cut into chunks of
 * min(64, SOLO_DEC_SCRATCH_CAP / (n_streams x 2216)) packets but never less than ONE, and the chunks of a call use the buffer one after the other, so it holds at most
 * max(n_streams x 2216 B, SOLO_DEC_SCRATCH_CAP bytes) (environment, read when the handle decodes for the first time; default -- also for 0 or an unparsable
 * value -- 1 GiB: 4096 streams x 64 packets are 581 MB, 8192 streams get chunks of 59 packets).
 * ---------------------------------------------------------------------------------------------- */
typedef struct solo_batch solo_batch_t;

#define SOLO_PACKET_SAMPLES 640
#define SOLO_DEFAULT_SLOT_BYTES 512

/* Creates encoder and/or decoder state for n_streams streams (pass NULL to skip one direction). */
solo_batch_t *solo_batch_create(int32_t n_streams, const USER_Ctrl_enc *enc, const USER_Ctrl_dec *dec,
                                int32_t slot_bytes);
void solo_batch_destroy(solo_batch_t *b);
/* Re-initialises all stream states (same as destroy + create) -- EXCEPT the receiver staging ring: descriptions filed with
 * solo_recv_insert, play-out positions and statistics survive a reset; call solo_recv_create again to start the ring afresh. */
int32_t solo_batch_reset(solo_batch_t *b, void *hip_stream);
/* Re-initialises the listed streams, each as AGR_Sate_Encoder_Init / AGR_Sate_Decoder_Init would with its own control.
 * which: 1 = encoder state, 2 = decoder state, 3 = both (only directions the handle has).  h_enc / h_dec: HOST arrays of n
 * controls, h_enc[i] for stream h_streams[i]; NULL = the handle's create-time control for that direction.  Other streams untouched.
 *   Per stream:  encoder targetRate_bps (<= 0 means 15600, AGR_BWE_SDK_API.c:35; the caller's array is not written back), dtx_enable,
 *                useMDIndex (mode is ignored, as in the reference); decoder useMDIndex (packetLoss_perc is ignored, as in the reference).
 *   Per handle:  samplerate, framesize_ms, joint_enable, joint_mode (they select the kernel build and the packet geometry): a listed
 *                control that differs from the handle's in any of them is refused.
 * Returns -1 and changes nothing (the checks run on the host before anything is enqueued) when n <= 0 or n > N, an index is out of
 * range or listed twice, `which` names a direction the handle does not have, a control is given for a direction the call does not
 * reset, or a control fails the checks of solo_batch_create (in the 32 kHz mode every stream's rate must leave SILK >= 14000 bps).
 * Ordering as solo_batch_reset: the init kernels wait for this handle's encode work still in flight on its internal streams
 * (async joins included) and for its latest decode call, whichever stream that was issued on; work enqueued on hip_stream after the call sees the new states.  The host arrays are free when the call
 * returns (the records travel as kernel arguments).  Reset streams play on with the receiver ring as it is: see solo_recv_reset_streams.
 * A handle created with one control and given per-stream controls here is the way to run mixed rates / DTX / useMDIndex in one batch. */
int32_t solo_batch_reset_streams(solo_batch_t *b, const int32_t *h_streams, int32_t n, int32_t which,
                                 const USER_Ctrl_enc *h_enc, const USER_Ctrl_dec *h_dec, void *hip_stream);
/* Changes the control of the listed RUNNING streams without re-initialising them: what SKP_Silk_SDK_Encode / _Decode take from their
 * control on every call (SKP_Silk_enc_API.c:165-176, SKP_Silk_dec_API.c:107).  Arguments, checks and refusals are exactly those of
 * solo_batch_reset_streams (-1 and nothing enqueued).
 *   Encoder, per stream:  the SILK rate (targetRate_bps, <= 0 meaning 15600, minus 1600 -- 800 with joint_mode 1 --, clamped to
 *                         [5000, 100000]) sets the two SNR targets as SKP_Silk_setup_rate_FIX does; dtx_enable and useMDIndex are set.
 *   Decoder, per stream:  useMDIndex is set.
 * Every other byte of the states stays bit for bit (first_frame_after_reset, VAD, noSpeechCounter / inDTX, all histories), and so do
 * the receiver ring and the play-out positions.  The new control applies from the first packet encoded / decoded after the call on
 * hip_stream; the update waits for this handle's encode / decode work still in flight (async joins included), so packets of earlier
 * calls keep the old control.  Side effects, as in the reference: DTX switched on during a silence of more than 5 frames drops the very
 * next packet (noSpeechCounter kept counting); sender and receiver must switch useMDIndex at the same packet; whether the receiver ring
 * files a desc = -1 arrival follows the stream's decoder useMDIndex when solo_recv_insert runs. */
int32_t solo_batch_update_streams(solo_batch_t *b, const int32_t *h_streams, int32_t n, int32_t which,
                                  const USER_Ctrl_enc *h_enc, const USER_Ctrl_dec *h_dec, void *hip_stream);
/* Graph capture.  solo_batch_encode, solo_batch_decode, solo_batch_decode_split, the subset calls, solo_batch_wait_encode,
 * solo_recv_insert, solo_recv_decode and the calls below that say so can be recorded into a graph (hipStreamBeginCapture on hip_stream,
 * torch.cuda.graph) and replayed; tests/test_gpu_graph_replay.py captures every one of them.  What holds for all of them:
 *   Set-up comes first.  A handle's FIRST encode call, its first decode call and solo_recv_create / solo_recv_track allocate, create
 *     streams and events and read the environment: they cannot run inside a capture.  The same goes for scratch: make one call of the
 *     same geometry (or of the largest the graph's life will see) before capturing.  A graph holds the ADDRESSES of the handle's scratch
 *     (hand-over records, extraction records, the mix / send scratch): any later call, captured or not, that is larger than every one
 *     before re-allocates it, and a graph captured earlier must then be captured again -- replaying it would write to freed memory.
 *   Frozen into the graph: every host argument -- n, n_packets, n_arrivals, payload_bytes, n_rooms, max_speakers, first_seq, min_ready,
 *     max_span, flags, the caps, the counts solo_playout_render takes, the parameter structs (they travel as kernel arguments) -- and
 *     the pointers.  A replay numbers its packets with the SAME first_seq: a tick that moves on brings d_seq_base and advances it on
 *     the device.  What a replay varies is the CONTENTS of device buffers: PCM, payloads, arrivals (pad a tick that brought fewer than
 *     n_arrivals with records of stream -1: they are counted `bad` and nothing else), the d_streams / d_rows lists, rooms, gains.
 *   Order.  The events by which one encode call of a handle waits for the one before (also across streams) are waited for only between
 *     calls of ONE context: both issued on running streams, or both inside the same capture; and the event a decode call leaves orders
 *     nothing outside the graph it was recorded in.  Across the boundary the stream is the order: a graph launch runs as a whole where it
 *     stands in its stream, so launch the replays and issue the eager calls of a handle on one stream, or order the streams yourself.  With asynchronous joins the solo_batch_wait_encode of a captured encode call
 *     belongs into the same capture.
 *   Schedules.  SOLO_ENC_PERSIST=1 does not survive a replay (its tickets are host counters passed by value: the second replay would
 *     find the first one's flags raised): such an encode call is refused inside a capture (-hipErrorStreamCaptureUnsupported).
 *     SOLO_ENC_GATE=1 replays correctly but stops gating: its targets are frozen while the device counters run on, so from the second
 *     replay on -- and for eager calls afterwards -- every gate opens at once (never the 20 ms bail-out).  solo_batch_set_timing
 *     brackets do not belong into a capture.
 *   Hardware queues.  An encode call of n_packets > 1 is a graph with parallel branches (three internal streams).  Operators report
 *     that the HIP runtime can crash replaying such a graph with fewer than 4 hardware queues (GPU_MAX_HW_QUEUES; not measured here). */
int32_t solo_batch_encode(solo_batch_t *b, const int16_t *d_pcm, int32_t n_packets, uint8_t *d_bits,
                          int16_t *d_nbytes, int32_t *d_status, void *hip_stream);
int32_t solo_batch_decode(solo_batch_t *b, const uint8_t *d_bits, const int16_t *d_nbytes,
                          const uint8_t *d_recv, int32_t n_packets, int16_t *d_pcm, int32_t *d_status,
                          void *hip_stream);
/* Receiver front end: the two descriptions of every packet arrive separately (MD1, and MD2 || HB(8)), possibly only one,
 * possibly in either arrival slot.  d_descA / d_descB: uint8 [N][P][slot_bytes]; d_lenA / d_lenB: int16 [N][P], 0 = nothing
 * arrived.  With useMDIndex = 1 in the stream's decoder control the kernel identifies the descriptions by the index they carry
 * (SKP_Silk_decode_parameters.c:55-57) and sorts them itself; with useMDIndex = 0 slot A is MD1 and slot B is MD2 || HB.
 * Builds the (ptr, nBytes, lostflag) call of test/dec_main.c:255-378 on the GPU and decodes.  Same outputs as
 * solo_batch_decode.  Packets above 252 bytes are rejected (status -11). */
int32_t solo_batch_decode_split(solo_batch_t *b, const uint8_t *d_descA, const int16_t *d_lenA, const uint8_t *d_descB,
                                const int16_t *d_lenB, int32_t slot_bytes, int32_t n_packets, int16_t *d_pcm,
                                int32_t *d_status, void *hip_stream);
/* Receiver staging ring: the "cache queue" of README.md:52-58 (imag/solo_neteq.png) kept in device memory for all streams of the
 * handle.  solo_recv_create: queue of `depth` sequence numbers per stream (1..4096), `slot_bytes` per description (<= 32767), every
 * stream's play-out position at `first_seq` (>= 0); calling it again empties the queue.  solo_recv_insert files n arrivals in any
 * order: stream, sequence number of the 40 ms packet, desc = 0 (MD1) / 1 (MD2 || HB) when the transport knows which description it
 * carries, -1 when it does not (the library reads the index the description carries as its first coded symbol: needs
 * useMDIndex = 1), payload = d_payload[offset .. offset + len).  An arrival for a packet that has been played, that lies `depth` or
 * more ahead, whose slot is taken (a second copy) or whose fields are out of range is dropped and counted.  solo_recv_decode decodes the
 * next n_packets (<= depth) sequence numbers of EVERY stream from what has arrived by then (the merge and the (ptr, nBytes, lostflag)
 * mapping of solo_batch_decode_split; nothing arrived = concealment), frees those entries and advances the play-out positions.
 * Like solo_batch_decode_split it refuses a packet whose descriptions together exceed 252 bytes: not decoded, d_status -11.
 * d_pcm int16 [N][n_packets][packet samples], d_status int32 [N] or NULL.  Calls on one handle must be ordered (same stream, or
 * events).  solo_recv_stats copies {inserted, late, ahead, duplicate, bad, 0, 0, 0} to HOST memory (synchronises the stream).
 * solo_recv_insert and solo_recv_decode enqueue kernels on hip_stream only and can be captured (n_arrivals, payload_bytes and n_packets are
 * frozen); solo_recv_create and solo_recv_stats cannot. */
typedef struct { int32_t stream, seq, desc, offset, len; } solo_arrival_t;
int32_t solo_recv_create(solo_batch_t *b, int32_t depth, int32_t slot_bytes, int32_t first_seq, void *hip_stream);
int32_t solo_recv_insert(solo_batch_t *b, const solo_arrival_t *d_arrivals, int32_t n_arrivals, const uint8_t *d_payload,
                         int64_t payload_bytes, void *hip_stream);
int32_t solo_recv_decode(solo_batch_t *b, int32_t n_packets, int16_t *d_pcm, int32_t *d_status, void *hip_stream);
int32_t solo_recv_stats(solo_batch_t *b, uint32_t *out8, void *hip_stream);
/* Receiver ring: empties the queue of the listed streams and sets their play-out positions to h_first_seq[i] (>= 0).
 * Statistics and all other streams are untouched.  h_streams / h_first_seq: HOST arrays of n; -1 (nothing changed) without a ring,
 * for n <= 0 or n > N, an index out of range or listed twice, or a negative sequence number.  Whether an arrival with desc = -1 is
 * accepted follows each stream's own decoder useMDIndex (solo_batch_reset_streams). */
int32_t solo_recv_reset_streams(solo_batch_t *b, const int32_t *h_streams, int32_t n, const int32_t *h_first_seq,
                                void *hip_stream);
/* Subset calls: encode, decode or play out only the n streams listed in d_streams, so that idle slots of a handle cost nothing.
 *   d_streams  int32 [n]  DEVICE array, strictly increasing, every index in [0, N).  Being on the device, a per-tick list needs no
 *                         host copy and the call can be captured in a graph (n itself is frozen: a replay brings other contents,
 *                         not another length).
 *   I/O is COMPACT: row i of d_pcm, d_bits, d_nbytes, d_recv and d_status belongs to stream d_streams[i] (shapes as in the
 *   calls above with n in place of N).  The codec state, the decoder state, the receiver queue and the play-out position are
 *   those of stream d_streams[i].  A listed stream moves on exactly as if it had been called alone; an UNLISTED stream keeps its
 *   encoder state, decoder state, receiver queue and play-out position bit for bit.
 * The host checks only 0 < n <= N and the pointers (-1 otherwise, nothing enqueued).  The list itself is checked on the device, on
 * hip_stream ahead of the call's kernels: a list that is not strictly increasing inside [0, N) is REFUSED -- no state, queue or
 * play-out position changes, the outputs are left untouched, and every d_status[i] (if d_status is given) is set to -1.
 * solo_batch_encode_streams always runs the launch-per-chunk schedule (SOLO_ENC_PERSIST does not apply to it); asynchronous joins and
 * solo_batch_wait_encode work as for solo_batch_encode.  It returns -1 when N x (the size of one stream's encoder state) reaches
 * 4 GiB (the quantiser addresses listed states with 32-bit offsets; ~249 000 streams at the 16 kHz API rate).
 * solo_batch_decode_streams sizes its extraction records by n (the chunking of solo_batch_decode with n streams).
 * solo_recv_decode_streams plays out the next n_packets sequence numbers of the listed streams only; the others keep their queue,
 * which is decoded later at its own sequence numbers.  Arrivals are filed with solo_recv_insert as before. */
int32_t solo_batch_encode_streams(solo_batch_t *b, const int32_t *d_streams, int32_t n, const int16_t *d_pcm, int32_t n_packets,
                                  uint8_t *d_bits, int16_t *d_nbytes, int32_t *d_status, void *hip_stream);
int32_t solo_batch_decode_streams(solo_batch_t *b, const int32_t *d_streams, int32_t n, const uint8_t *d_bits,
                                  const int16_t *d_nbytes, const uint8_t *d_recv, int32_t n_packets, int16_t *d_pcm,
                                  int32_t *d_status, void *hip_stream);
int32_t solo_recv_decode_streams(solo_batch_t *b, const int32_t *d_streams, int32_t n, int32_t n_packets, int16_t *d_pcm,
                                 int32_t *d_status, void *hip_stream);
/* Read side of the receiver ring: what is queued for a stream, what became of its arrivals and of its played packets, and -- from the
 * same pass -- the compacted list of the streams that are ready to play, in the form solo_recv_decode_streams takes.  The ring still
 * decides nothing (no play-out adaptation, no time stretching); it states the facts a jitter policy and a receiver report need.
 *   Queue fields (always): for stream s with play-out position p and ring depth D, from the D length words of the stream alone (a second
 *   description of <= hbb bytes, or a packet above 252 bytes that play-out will answer with -11, counts as queued like any other):
 *   play = p; queued / complete = sequence numbers of [p, p + D) that hold at least one / both descriptions; ready = length of the run
 *   of non-empty entries that starts AT p; span = 1 + (highest queued sequence number - p), 0 for an empty queue; head = entry p in
 *   d_recv format (bit 0 MD1 queued, bit 1 MD2 || HB queued).
 *   Counters (uint32, wrapping, cumulative; counted only while solo_recv_track is on): inserted / late / ahead / duplicate / bad = the
 *   verdict solo_recv_insert gave each arrival of the stream (an arrival whose stream index is out of range appears in solo_recv_stats
 *   only; solo_recv_stats itself is unchanged); played_both / played_md1 / played_md2 / played_none = one per packet that solo_recv_decode /
 *   solo_recv_decode_streams played for the stream, by its entry's length word at play-out (a refused list plays and counts nothing);
 *   margin_min = the smallest (seq - play) of an INSERTED arrival at filing time, D when there was none.  A handle that never tracked
 *   reports 0 everywhere and margin_min = D.
 * solo_recv_track(b, 1, st) allocates the counters on first use (40 bytes per stream) and ZEROES them on every call; (b, 0, st) stops
 * the counting and keeps the values (reports go on showing them).  -1 without a ring.  solo_recv_create zeroes the counters of all
 * streams and leaves the switch as it is; solo_recv_reset_streams zeroes those of the listed streams (a new call joins the slot).
 * Default: off -- solo_recv_insert and solo_recv_decode* then enqueue exactly the kernels they always did; on costs one more short
 * kernel per play-out call, ahead of the decoder.
 * solo_recv_report: row i is stream d_streams[i] (DEVICE list as in the subset calls), or stream i with d_streams = NULL and n = N.
 *   Row i is SELECTED iff ready_i >= m_i, m_i = d_min_ready ? d_min_ready[i] : min_ready (d_min_ready: DEVICE int32 [n] or NULL;
 *   m_i <= 0 selects always), or max_span > 0 and span_i >= max_span (the queue is about to overflow).
 *   d_reports   solo_recv_report_t [n], 16-byte aligned; d_play_list / d_play_rows int32 [n]: the stream index / the row index of the k-th
 *   selected row in row order, compacted, no holes; entries at and beyond `selected` are not written.  The input list is strictly
 *   increasing, so d_play_list is too: a valid d_streams of solo_recv_decode_streams.  d_count = {selected, n}; the caller reads these
 *   8 bytes to get the n of the play-out call.  Any of the three outputs may be NULL (not wanted).
 *   flags: SOLO_RECV_REPORT_CLEAR_MARGIN sets margin_min of the listed streams back to D after it was read.
 * Returns -1 with nothing enqueued for a NULL handle, no ring, n <= 0, n > N, d_streams = NULL with n != N, all three outputs NULL, a
 * list output without d_count, a d_reports that is not 16-byte aligned, unknown flag bits.  The list is checked on the device like that
 * of the other subset calls: one that is not strictly increasing inside [0, N) writes d_count->selected = -1 (when given) and nothing
 * else, and clears no margin.  At most three short kernels on hip_stream only, no host synchronisation, no allocation: the call can be
 * captured.  Calls on one handle must be ordered (same stream, or events), as for the rest of the ring. */
typedef struct {                 /* 64 bytes, one per listed stream */
    int32_t  play;               /* sequence number the stream decodes next                                             */
    int32_t  queued;             /* sequence numbers in [play, play + depth) that hold at least one description          */
    int32_t  complete;           /* of those, how many hold both                                                         */
    int32_t  ready;              /* length of the run of non-empty entries that starts AT play (0 .. depth)              */
    int32_t  span;               /* 1 + (highest queued sequence number - play); 0 when nothing is queued                */
    int32_t  head;               /* entry `play` in d_recv format: bit 0 MD1 queued, bit 1 MD2 || HB queued              */
    uint32_t inserted, late, ahead, duplicate, bad;           /* what became of this stream's arrivals (tracking on)     */
    uint32_t played_both, played_md1, played_md2, played_none;/* what its played packets were made of (tracking on)      */
    int32_t  margin_min;         /* smallest (seq - play) of an INSERTED arrival since the last clear; depth = none      */
} solo_recv_report_t;
typedef struct { int32_t selected, listed; } solo_recv_report_count_t;   /* 8 bytes; selected = -1: list refused on the device */

#define SOLO_RECV_REPORT_CLEAR_MARGIN 1

int32_t solo_recv_track(solo_batch_t *b, int32_t on, void *hip_stream);
int32_t solo_recv_report(solo_batch_t *b, const int32_t *d_streams, int32_t n,
                         const int32_t *d_min_ready, int32_t min_ready, int32_t max_span, int32_t flags,
                         solo_recv_report_t *d_reports, int32_t *d_play_list, int32_t *d_play_rows,
                         solo_recv_report_count_t *d_count, void *hip_stream);
/* Sender back end: turns what an encode call wrote into the datagrams that go on the wire -- per packet up to two, MD1 and
 * MD2 || HB -- as one solo_arrival_t per datagram plus a dense payload pool: exactly what solo_recv_insert of the receiving handle
 * takes, so encode -> pack -> (network, or another handle's ring) -> play-out never brings codec data to the host, and a
 * device-to-host copy of the result moves the bytes that are sent instead of whole slots.
 *   d_bits, d_nbytes  what solo_batch_encode / solo_batch_encode_streams wrote ([n][P][slot], [n][P][2]; compact rows in the _streams form)
 *   d_send            uint8 [n][P] in the format of d_recv: bit 0 sends MD1, bit 1 sends MD2 || HB; NULL = both.  Loss, single-description
 *                     and FEC policies are expressed through this mask.
 *   sequence number   of packet p of row i: first_seq + (d_seq_base ? d_seq_base[i] : 0) + p (d_seq_base: int32 [n] or NULL).  A packet
 *                     that is not sent still consumes its number: the ring counts packets, not datagrams.
 *   d_records         solo_arrival_t [max_records]: stream (i, or d_streams[i]), seq, desc (0 / 1), offset, len -- compacted, no holes
 *   d_payload         uint8 [payload_capacity]: the datagrams back to back, each offset the sum of the earlier lengths, no padding
 *   d_count           one solo_send_count_t (8-byte aligned): what was written and what the call needed, so that a caller whose buffers
 *                     were too small can size them and repeat the call
 * Order: PACKET-MAJOR (p outer), then row i, then description 0 before 1 -- a tick's datagrams are contiguous and the output is a pure
 * function of the inputs.  Which datagrams a packet yields, with hbb = 8, or 4 with framesize_ms 20 or joint_mode 1 (the geometry of the
 * handle: of its encoder, or of its decoder when it has no encoder), total = nbytes[0], n1 = nbytes[1]:
 *   total <= 0 (a DTX packet): none, counted `empty` -- whatever else the record says;
 *   a sequence number that is negative or does not fit int32, total > slot, n1 < 0, n1 > total or 0 < n1 < hbb: none, counted `refused`;
 *                     such a record is never dereferenced;
 *   otherwise         MD1 = the first total - n1 bytes if that is > 0 and bit 0 is set; MD2 || HB = the last n1 bytes if n1 > hbb and bit 1
 *                     is set.  Bytes of a slot beyond its payload are never read.
 * Record k is written iff k < max_records and offset_k + len_k <= min(payload_capacity, 2^31 - 1); both grow along the order, so what is
 * written is a prefix, and nothing is written at or beyond either cap (max_records = 0 / payload_capacity = 0 only count).  Sizes that
 * never overflow: 2 x n x n_packets records, n x n_packets x slot bytes.
 * Returns -1 with nothing enqueued for a NULL handle, d_bits, d_nbytes, d_records, d_payload or d_count, n_packets <= 0, a negative
 * cap, n x n_packets x 2 >= 2^31, and (_streams form) a NULL list or n outside (0, N].  The list itself is checked on the device like
 * that of the other subset calls: a list that is not strictly increasing inside [0, N) writes d_count->records = -1 and nothing else.
 * Any handle will do (only N, slot_bytes and the packet geometry are used; no codec state is read).  Three short kernels on hip_stream
 * only, no host synchronisation, so the call can be captured in a graph -- except that the handle's scratch for the scan (32 bytes per
 * 256 packets) grows, with a stream synchronisation, when a call is larger than every one before it.  The call does NOT wait for the
 * handle's internal streams: after an encode with asynchronous joins call solo_batch_wait_encode(b, hip_stream, 0) first.  Calls on
 * one handle must be ordered (same stream, or events). */
typedef struct {
    int32_t records, records_needed;   /* written / what the call would have written without the caps */
    int64_t bytes, bytes_needed;       /* the same for payload bytes */
    int32_t empty, refused;            /* packets skipped: total <= 0 (DTX) / sequence number or length record invalid */
} solo_send_count_t;                   /* 32 bytes */
int32_t solo_send_pack(solo_batch_t *b, const uint8_t *d_bits, const int16_t *d_nbytes, const uint8_t *d_send,
                       int32_t n_packets, const int32_t *d_seq_base, int32_t first_seq,
                       solo_arrival_t *d_records, int32_t max_records, uint8_t *d_payload, int64_t payload_capacity,
                       solo_send_count_t *d_count, void *hip_stream);
int32_t solo_send_pack_streams(solo_batch_t *b, const int32_t *d_streams, int32_t n, const uint8_t *d_bits, const int16_t *d_nbytes,
                               const uint8_t *d_send, int32_t n_packets, const int32_t *d_seq_base, int32_t first_seq,
                               solo_arrival_t *d_records, int32_t max_records, uint8_t *d_payload, int64_t payload_capacity,
                               solo_send_count_t *d_count, void *hip_stream);
/* Mixing bridge: the step between the receiving and the sending half -- every participant of a conference room hears the sum of the
 * others ("mix-minus"), on the device.  d_pcm_in / d_pcm_out: int16 [n][n_packets][L], L = the handle's packet samples: the layout the
 * decode calls write and the encode calls read, compact rows of the subset calls included (the mixer works on ROWS and never looks at
 * slot numbers).  d_room: int32 [n], the room of row i in [0, n_rooms), or -1 = in no room.  d_gain_q12: int16 [n] or NULL (= 4096
 * everywhere); a negative gain counts as 0.  Per packet p, statelessly, for a room with member set M:
 *   c_j[s]   = (x_j[s] * g_j + 2048) >> 12            (arithmetic shift; g = 4096 passes the samples through)
 *   e_j      = sum_s c_j[s]^2                          (64 bits, exact)
 *   sel      = M when max_speakers <= 0 or >= |M|, else the max_speakers members that come first in the order
 *              (larger e_j first, then smaller row index)
 *   S[s]     = sum_{j in sel} c_j[s]
 *   out_i[s] = sat16(S[s] - (i in sel ? c_i[s] : 0))   for every i in M -- a room of one hears silence.
 * d_energy (int64 [n][n_packets] or NULL): e_j; d_mixed (uint8 [n][n_packets] or NULL): 1 if the row was in sel.  Rows with room -1:
 * nothing of d_pcm_out, d_energy, d_mixed is written.  d_count (may be NULL): rows that got an output, rooms with at least one member,
 * output samples that saturated.
 * Returns -1 with nothing enqueued for a NULL handle, d_pcm_in, d_room or d_pcm_out; n <= 0, n_packets <= 0, n_rooms <= 0 or > n;
 * n x n_packets >= 2^31; max_speakers > 64; max_speakers <= 0 together with n > 8191 (only then could more than 8191 contributions of
 * |c| < 2^18 meet in one 32-bit sum; a caller with more rows passes max_speakers 64, which still mixes every member of any room of up
 * to 64); PCM pointers that are not 16-byte aligned; input and output ranges that overlap (mix-minus cannot run in place).
 * A room id outside [-1, n_rooms) is found on the device, ahead of the other kernels, and refuses the whole call: nothing is written
 * except d_count->rows = -1.
 * Any handle will do (only L and the handle's scratch are used).  Five short kernels on hip_stream only, no host synchronisation, so
 * the call can be captured in a graph -- except that the handle's scratch for the room plan (9 bytes per row and packet + 16 per row)
 * grows, with a stream synchronisation, when a call is larger than every one before it.  Like solo_send_pack the call does NOT wait
 * for the handle's internal streams, and calls on one handle must be ordered.  One wavefront walks a (room, packet): a room of
 * thousands is mixed correctly but not in parallel (INTEGRATION.md section 2 has the measured costs). */
typedef struct {
    int32_t rows, rooms;   /* rows that got an output / rooms with at least one member; rows = -1: call refused on the device */
    int64_t clipped;       /* output samples that saturated */
} solo_mix_count_t;        /* 16 bytes */
int32_t solo_mix(solo_batch_t *b, const int16_t *d_pcm_in, int32_t n, int32_t n_packets,
                 const int32_t *d_room, int32_t n_rooms, const int16_t *d_gain_q12, int32_t max_speakers,
                 int16_t *d_pcm_out, int64_t *d_energy, uint8_t *d_mixed,
                 solo_mix_count_t *d_count, void *hip_stream);
/* Mixing bridge with SHARED listener mixes: with max_speakers = k every member of a room that is not among the picked speakers hears the
 * same samples, sat16(S), so this form writes that row once per room and a personal row only per speaker -- the encoder behind it then runs
 * once per speaker and once per room instead of once per listener.  c_j, e_j, sel (per room and packet) and S are EXACTLY those of solo_mix
 * (same arithmetic, same order: larger energy first, then smaller row index); max_speakers must be in [1, 64], so the 8191-row limit of the
 * mix-everyone form does not apply.  d_pcm_in, d_room, n_rooms, d_gain_q12, d_energy, d_mixed: as for solo_mix.
 *   speaker of the call   a row in a room that is in sel in at least one of the call's packets, or whose d_keep[i] != 0 (d_keep: uint8 [n] or
 *                         NULL -- the caller's hangover policy: a row keeps its own encoder for a while after it stopped talking)
 *   shared room           a room with at least one member that is not a speaker of the call
 *   d_pcm_spk   int16 [n][P][L], only the first `speakers` rows are written: row k belongs to the k-th speaker i in increasing row order,
 *               packet p of it is sat16(S_p - (i in sel_p ? c_i : 0))
 *   d_spk_rows  int32 [n] or NULL: d_spk_rows[k] = i
 *   d_spk_list  int32 [n]: d_spk_list[k] = d_slots ? d_slots[i] : i.  d_slots (int32 [n] or NULL) maps rows to transmit slots, strictly
 *               increasing and non-negative (the list the rows were decoded by); the list is then strictly increasing: a valid d_streams of
 *               solo_batch_encode_streams on the participants' handle
 *   d_pcm_room  int16 [n_rooms][P][L], only the first `shared` rows are written: row j belongs to the j-th shared room in increasing room
 *               order, packet p of it is sat16(S_p)
 *   d_room_list int32 [n_rooms]: d_room_list[j] = that room's id; strictly increasing: a valid d_streams on a second handle with one slot per room
 *   d_source    int32 [n]: k for a speaker, n + j for any other member of the j-th shared room, -1 for a row in no room.  With the encoded
 *               speakers in rows 0.. and the encoded rooms in rows n.. of ONE table this is the d_source of solo_send_fanout.
 *   d_count     rows, rooms as for solo_mix; speakers, shared; clipped: saturated samples among the rows that were written
 * Nothing beyond the counts is written (rows `speakers`.. of d_pcm_spk, d_spk_list, d_spk_rows, rows `shared`.. of d_pcm_room, d_room_list),
 * and of d_energy / d_mixed nothing for rows in no room.
 * Returns -1 with nothing enqueued for everything solo_mix refuses; max_speakers outside [1, 64]; a NULL d_pcm_spk, d_spk_list, d_pcm_room,
 * d_room_list, d_source or d_count; PCM outputs that are not 16-byte aligned or overlap the input or each other.  A room id outside
 * [-1, n_rooms) or a d_slots that is not strictly increasing from a non-negative start is found on the device, ahead of the other kernels:
 * nothing is written except d_count->rows = -1.
 * Any handle will do.  Ten short kernels on hip_stream only, no host synchronisation, capturable -- except that the handle's scratch (the
 * one of solo_mix; 13 bytes per row and packet + 28 per row) grows, with a stream synchronisation, when a call is larger than every one
 * before it.  The energies are computed by one wavefront per (row, packet), so one room of thousands costs what thousands of small rooms
 * cost.  The call does not wait for the handle's internal streams, and calls on one handle must be ordered. */
typedef struct {
    int32_t rows, rooms;        /* as solo_mix_count_t; rows = -1: call refused on the device */
    int32_t speakers, shared;   /* rows of d_pcm_spk / d_pcm_room that were written */
    int64_t clipped;            /* samples of those rows that saturated */
} solo_mix_shared_count_t;     /* 24 bytes */
int32_t solo_mix_shared(solo_batch_t *b, const int16_t *d_pcm_in, int32_t n, int32_t n_packets,
                        const int32_t *d_room, int32_t n_rooms, const int16_t *d_gain_q12, int32_t max_speakers,
                        const uint8_t *d_keep, const int32_t *d_slots,
                        int16_t *d_pcm_spk, int32_t *d_spk_list, int32_t *d_spk_rows,
                        int16_t *d_pcm_room, int32_t *d_room_list, int32_t *d_source,
                        int64_t *d_energy, uint8_t *d_mixed,
                        solo_mix_shared_count_t *d_count, void *hip_stream);
/* Shared listener mixes from a GIVEN selection: solo_mix_shared for a bridge that has already decided who speaks (solo_vad_select, or any
 * policy of its own).  Everything is as in solo_mix_shared except where the selection comes from: there is no max_speakers, no energy is
 * needed, and a room may have no speaker at all.  d_pcm_in, n, n_packets, d_room, n_rooms, d_keep, d_slots and the layouts and ordering
 * rules of d_pcm_spk, d_spk_list, d_spk_rows, d_pcm_room, d_room_list and d_source: as there, so they feed solo_batch_encode_streams and
 * solo_send_fanout unchanged.  d_gain_q12 is the callers' own gains (not the masked d_gain_out of solo_vad_select).
 *   d_sel       uint8 [n][P], required: exactly what solo_vad_select writes to its d_sel.  sel_p(r) = { i in room r : d_sel[i][p] != 0 }; it
 *               may be empty and it may hold every member; a non-zero entry of a row in no room is ignored
 *   c_j         solo_mix's;  S_p = sum over sel_p of c_j (at most 64 terms of |c| < 2^18: the 32-bit sum is exact and independent of the order)
 *   speaker of the call   a row that is in sel_p for at least one p, or whose d_keep[i] != 0.  A selected row with gain 0 is a speaker: the
 *               selection is taken as given
 *   shared room a room with at least one member that is not a speaker of the call
 *   d_pcm_spk   packet p of speaker i is sat16(S_p - (i in sel_p ? c_i : 0))
 *   d_pcm_room  packet p of a shared room is sat16(S_p)
 *   d_room_nsel uint8 [n_rooms][P] or NULL, only the first `shared` rows are written: [j][p] = |sel_p| of the j-th shared room.  0 means that
 *               packet of d_pcm_room[j] is all zeros: the caller may clear that destination's bits in the d_send mask of solo_send_fanout,
 *               or let DTX handle it
 *   d_energy    int64 [n][P] or NULL: solo_mix's e_j.  NULL: the energy pass, one full read of the input, is not launched at all
 *   d_count     rows, rooms, speakers, shared, clipped as for solo_mix_shared; selected: (row, packet) pairs selected among rows in a room;
 *               silent: (shared room, packet) pairs with an empty selection
 * There is no d_mixed: it would be d_sel.
 * Returns -1 with nothing enqueued for everything solo_mix_shared refuses (max_speakers does not exist here); a NULL d_sel; PCM outputs that
 * are not 16-byte aligned or overlap the input or each other.  Found on the device, ahead of anything written to a caller's buffer (d_energy
 * included): a room id outside [-1, n_rooms); a d_slots that does not grow strictly from a non-negative start; more than 64 selected
 * members in any one (room, packet).  Nothing is then written except d_count->rows = -1.
 * Any handle will do.  Nine short kernels (ten with d_energy) on hip_stream only, no host synchronisation, capturable -- except that the
 * handle's scratch (the one of solo_mix; here 8 bytes per row and packet + 28 per row) grows, with a stream synchronisation, when a call is
 * larger than every one before it.  The call does not wait for the handle's internal streams, and calls on one handle must be ordered.
 * INTEGRATION.md section 2 has the tick. */
typedef struct {
    int32_t rows, rooms;        /* as solo_mix_count_t; rows = -1: call refused on the device */
    int32_t speakers, shared;   /* rows of d_pcm_spk / d_pcm_room that were written */
    int64_t clipped;            /* samples of those rows that saturated */
    int32_t selected, silent;   /* (row, packet) pairs selected among rows in a room / (shared room, packet) pairs with an empty selection */
} solo_mix_selected_count_t;   /* 32 bytes */
int32_t solo_mix_selected(solo_batch_t *b, const int16_t *d_pcm_in, int32_t n, int32_t n_packets,
                          const int32_t *d_room, int32_t n_rooms, const int16_t *d_gain_q12, const uint8_t *d_sel,
                          const uint8_t *d_keep, const int32_t *d_slots,
                          int16_t *d_pcm_spk, int32_t *d_spk_list, int32_t *d_spk_rows,
                          int16_t *d_pcm_room, int32_t *d_room_list, int32_t *d_source,
                          uint8_t *d_room_nsel, int64_t *d_energy,
                          solo_mix_selected_count_t *d_count, void *hip_stream);
/* Sender back end for shared sources: ONE table of encoded packets (d_bits [n_src][P][slot], d_nbytes [n_src][P][2], the layout the encode
 * calls write), MANY destinations.  Destination i of n_dst sends the packets of source row d_source[i] (-1: it sends nothing and is not
 * counted) as stream d_dst_stream ? d_dst_stream[i] : i, with the sequence numbers first_seq + (d_seq_base ? d_seq_base[i] : 0) + p and under
 * the mask d_send[i][p] (uint8 [n_dst][P], bit 0 = MD1, bit 1 = MD2 || HB, NULL = both).  The send step behind solo_mix_shared, and a
 * forwarding server's copy of one sender to many receivers without transcoding.
 * Which datagrams a source packet yields, and when it counts as `empty` or `refused`, are the rules of solo_send_pack applied to the
 * source's length record with the destination's mask and sequence number; empty / refused are counted once per (destination, packet).
 *   pool      every source datagram is stored ONCE: the valid datagrams (both descriptions, whatever the masks say) of every source row that
 *             at least one destination names, back to back, per packet (outer), then source row, then description 0 before 1.  Rows nobody
 *             names are never read -- in the bridge their length words are uninitialised.
 *   records   per packet (outer), then destination i, then description 0 before 1: {stream, seq, desc, offset of the shared datagram, len}.
 *             Records of destinations with one source carry the same offset; solo_recv_insert files every one of them.
 * A pool datagram is written iff it ends inside min(payload_capacity, 2^31 - 1) -- a prefix of the pool; record k is written iff
 * k < max_records and its datagram was.  (A byte cap that cuts inside a packet's pool can therefore leave holes among that packet's
 * records; the record cap alone cuts a prefix.)  d_count: records / bytes written, records_needed / bytes_needed (the pool's) without the
 * caps; caps of 0 only count.
 * Returns -1 with nothing enqueued for a NULL handle, d_bits, d_nbytes, d_source, d_records, d_payload or d_count; n_src, n_dst or
 * n_packets <= 0; a negative cap; n_dst x n_packets x 2 >= 2^31 or n_src x n_packets x 2 >= 2^31.  A d_source entry outside [-1, n_src) is
 * found on the device, ahead of the other kernels: nothing is written except d_count->records = -1.
 * Any handle will do (slot_bytes and the packet geometry are used, and the scratch of solo_send_pack: 8 bytes per source packet, 4 per source
 * row and 24 per 256 packets, grown as there).  Six short kernels on hip_stream only, no host synchronisation, so the call can be captured like
 * solo_send_pack; the call does not wait for the handle's internal streams, and calls on one handle must be ordered. */
int32_t solo_send_fanout(solo_batch_t *b, const uint8_t *d_bits, const int16_t *d_nbytes, int32_t n_src,
                         const int32_t *d_source, const int32_t *d_dst_stream, int32_t n_dst,
                         const uint8_t *d_send, int32_t n_packets, const int32_t *d_seq_base, int32_t first_seq,
                         solo_arrival_t *d_records, int32_t max_records, uint8_t *d_payload, int64_t payload_capacity,
                         solo_send_count_t *d_count, void *hip_stream);
/* Play-out time scaling by whole packets: the step between play-out and mix that MOVES a stream's play-out delay -- in_packets = a decoded
 * packets of a row become out_packets = b packets of audio without a click (waveform-similarity overlap-add).  d_pcm_in: int16 [n][a][L],
 * d_pcm_out: int16 [n][b][L], L = the handle's packet samples: the compact rows every other call reads and writes.  Integer arithmetic with
 * a total order for every choice: the output is a pure function of the input.  Per row, statelessly: input x[0 .. Li), Li = a L; output
 * y[0 .. Lo), Lo = b L; H = samplerate / 200 (5 ms: 80 or 160 samples), D = 3H / 2, M = Lo / H output blocks, j = 0 .. H - 1.
 *   n_m    = floor((2 m (Li - H) + (M - 1)) / (2 (M - 1)))     the nominal source position of block m: n_0 = 0, n_{M-1} = Li - H
 *   block 0:          y[j] = x[j], s_0 = 0
 *   blocks m >= 1:    the template t[j] = x[s_{m-1} + H + j]: what the previous block's segment would have played next
 *   1 <= m <= M - 2:  the candidates are every d in [max(-D, -n_m), min(D, Li - 2H - n_m)] (never fewer than 57),
 *                       cost(d) = sum_j |t[j] - x[n_m + d + j]|
 *                               + sum_j |x[n_m + d + H + j] - x[Li - H + j]|    for m = M - 2 only: how the candidate's own continuation
 *                                                                               meets the pinned last block
 *                     d_m = the candidate with the least (cost, |d|, d) in lexicographic order; s_m = n_m + d_m
 *   m = M - 1:        s_m = Li - H (pinned), d_m = 0, cost = sum_j |t[j] - x[s_m + j]|
 *   blocks m >= 1:    y[m H + j] = floor((t[j] (H - 1 - j) + x[s_m + j] (j + 1) + H / 2) / H)      (floor towards minus infinity)
 * So the first H output samples are the input's first H and the last output sample is the input's last: a row joins the packets played
 * before and after it exactly as the unscaled signal would.  a == b is the identity (every d_m = 0, every cost 0).  No output sample
 * leaves the range of its two sources: nothing saturates.  A cost is at most 2 H 65535 < 2^25.
 * d_shift, d_cost (int32 [n][M] or NULL): d_m and the least cost of block m (the cost above, second term included at m = M - 2); 0 for
 * block 0.  They are the caller's quality gate: a row whose splices were expensive can be played unscaled instead.  d_count (may be
 * NULL): rows written, blocks searched (n (M - 2)), the sum of all costs.
 * Returns -1 with nothing enqueued for a NULL handle, d_pcm_in or d_pcm_out; n <= 0; in_packets or out_packets outside 1 .. 4;
 * n x max(a, b) x L >= 2^31; PCM pointers that are not 16-byte aligned; input and output ranges that overlap.
 * Any handle will do (only L and the sample rate are read).  No scratch, no allocation, no host synchronisation: one kernel on hip_stream
 * (one wavefront per row; a second, one-lane kernel ahead of it when d_count is given), so the call can be captured in a graph.  Like
 * solo_mix it does NOT wait for the handle's internal streams.  The policy -- when to scale which stream -- is the caller's
 * ("Moving a stream's play-out delay"). */
typedef struct { int32_t rows, blocks; int64_t cost; } solo_timescale_count_t;   /* 16 bytes: rows written, blocks searched, sum of all splice costs */
int32_t solo_timescale(solo_batch_t *b, const int16_t *d_pcm_in, int32_t n, int32_t in_packets, int32_t out_packets,
                       int16_t *d_pcm_out, int32_t *d_shift, int32_t *d_cost, solo_timescale_count_t *d_count, void *hip_stream);
/* PCM rate conversion on the device: the reference SDK's own fixed-point resampler (SKP_Silk_resampler_init / SKP_Silk_resampler), bit for
 * bit and with its stream state, so that callers on handles of different rates meet in one mix and 8 / 48 kHz endpoints need no host
 * round trip.  A resampler is an object of its own -- it sits BETWEEN two handles -- with n_rows independent rows of filter memory.
 *   pairs      fs_in -> fs_out with both rates in {8000, 16000, 32000, 48000} and fs_out : fs_in one of 1:2, 2:1, 1:3, 3:1, 2:3, 3:2:
 *              48->16, 48->32, 32->16, 16->8 (second-order AR filter + 12-tap FIR), 16->32, 8->16 (all-pass 2x up-sampler with notch),
 *              16->48, 32->48 (2x up-sampler + 6-tap fractional interpolation).  Every other pair -- equal rates, 1:4 (32->8), 1:6
 *              (48->8) and their inverses, 12 / 24 / 44.1 kHz, rates above 48 kHz -- makes the create call return NULL.
 *   d_in       int16 [n][n_packets][in_samples], d_out int16 [n][n_packets][out_samples]: the layouts the decode calls write and that
 *              the mixer and the encode calls read, compact rows of the subset calls included.  Both 16-byte aligned, not overlapping.
 *   in_samples any positive multiple of 10 ms of input (fs_in / 100 samples): a 20 ms or 40 ms packet at any of the four rates.  The
 *              output has exactly in_samples * fs_out / fs_in samples per packet (see the out_samples call, -1 off that grid).
 * The conversion works in batches of 10 ms as the reference does, so P packets in one call give what P calls of one packet give, and a
 * row's 96 bytes of filter memory (the reference's sIIR[6], sFIR[16], sDown2[2]; about 1 ms of signal) live in device memory inside the
 * object and carry from call to call.  The create call zeroes them (= the reference's init), and so do the two reset calls: every row,
 * or a HOST list of rows (1 .. n_rows indices inside [0, n_rows), none twice, else -1), as the per-stream reset of a batch handle.
 * The rows variant converts only the listed rows: d_rows is a DEVICE list, strictly increasing inside [0, n_rows), checked on the
 * device ahead of the work like the lists of the other subset calls; row i of d_in / d_out belongs to d_rows[i] (compact I/O); unlisted
 * rows keep their state bit for bit.  A refused list changes no state and writes nothing except d_count->rows = -1.
 * Return -1 with nothing enqueued: NULL pointers (d_count included, in the rows variant); n outside (0, n_rows]; n_packets <= 0;
 * in_samples not a positive multiple of fs_in / 100; n x n_packets x in_samples or x out_samples >= 2^31; buffers that are not 16-byte
 * aligned or that overlap.  One kernel (two with a list) on hip_stream only, no host synchronisation and no allocation: the calls can
 * be captured in a graph.  Calls on one resampler must be ordered (same stream, or events).
 * Not offered: the other ratios; sample formats other than int16; resampler state in a migration blob -- a row that moves to another
 * object starts from a reset there (its memory is about 1 ms of signal).  INTEGRATION.md section 2 has the recipes. */
typedef struct solo_resampler solo_resampler_t;
typedef struct { int32_t rows, listed; } solo_resample_count_t;   /* rows converted / rows listed; rows = -1: list refused on the device */
solo_resampler_t *solo_resample_create(int32_t n_rows, int32_t fs_in, int32_t fs_out);
void solo_resample_destroy(solo_resampler_t *r);
int32_t solo_resample_out_samples(const solo_resampler_t *r, int32_t in_samples);
int32_t solo_resample_reset(solo_resampler_t *r, void *hip_stream);
int32_t solo_resample_reset_rows(solo_resampler_t *r, const int32_t *h_rows, int32_t n, void *hip_stream);
int32_t solo_resample(solo_resampler_t *r, const int16_t *d_in, int32_t n_packets, int32_t in_samples,
                      int16_t *d_out, void *hip_stream);
int32_t solo_resample_rows(solo_resampler_t *r, const int32_t *d_rows, int32_t n, const int16_t *d_in, int32_t n_packets,
                           int32_t in_samples, int16_t *d_out, solo_resample_count_t *d_count, void *hip_stream);
/* Voice activity, audio level and speaker selection for decoded rows: who is speaking, with memory.  solo_mix and solo_mix_shared pick
 * by the energy of one packet, statelessly; these calls give a bridge the facts for a better decision without a host round trip.  A
 * solo_vad_t is an object of its own, like a resampler, with n_rows independent rows of state.
 *   frame_samples  320 (SILK's wide-band configuration: 20 ms at 16 kHz) or 160 (20 ms at 8 kHz); anything else: NULL.  A 32 kHz row
 *              either goes through solo_resample 32 -> 16 first, or runs 320-sample frames of 10 ms: every time constant of the noise
 *              tracker then runs twice as fast.
 *   state      SOLO_VAD_STATE_BYTES = 128 bytes per row in device memory.  Bytes [0, 112) are the reference's SKP_Silk_VAD_state in its
 *              own layout -- AnaState[2], AnaState1[2], AnaState2[2], XnrgSubfr[4], NrgRatioSmth_Q8[4], HPstate (int16 + 2 zero bytes),
 *              NL[4], inv_NL[4], NoiseLevelBias[4], counter --, bytes [112, 128) the selection state {int32 talking, hang, picked, 0}.
 *              Create and the two reset calls (every row, or a HOST list of 1 .. n_rows indices inside [0, n_rows), none twice, else -1)
 *              leave what SKP_Silk_VAD_Init leaves, selection state zero.  solo_vad_get_state / solo_vad_set_state copy the records
 *              of listed rows to / from d_blob, uint8 [n][128] (4-byte aligned): d_rows is a DEVICE list, or NULL for rows 0 .. n - 1;
 *              plain copies -- an index outside [0, n_rows) moves nothing.  They are what a migrating call takes along (VAD state is
 *              not part of a migration blob).
 * solo_vad: d_pcm is int16 [n][n_packets][packet_samples], the compact rows every other call reads and writes; packet_samples is a
 *   positive multiple of frame_samples and at most 1920, F = packet_samples / frame_samples.  Frame by frame, in order, the call does
 *   exactly what SKP_Silk_VAD_GetSA_Q8(state, ..., frame, frame_samples) does, bit for bit: d_sa_q8 (uint8 [n][P][F]) receives *pSA_Q8,
 *   d_detail (int32 [n][P][F][6] or NULL) {SNR_dB_Q7, Tilt_Q15, Quality_Q15[0 .. 3]}.  The state carries from frame to frame and from
 *   call to call: P packets in one call equal P calls of one packet.
 *   d_level (uint8 [n][P] or NULL) is the RFC 6464 audio level of each packet in -dBov, 0 = loudest -- what goes into the RTP audio-level
 *   header extension: E = sum x^2, exact in 64 bits; level = the smallest k in [0, 127] with E * 2^20 >= packet_samples * T_k,
 *   T_k = round(2^50 * 10^(-k / 10)); 127 if there is none.  (All products fit 64 unsigned bits at packet_samples <= 1920.)
 *   With d_rows (a DEVICE list, strictly increasing inside [0, n_rows), checked on the device ahead of the work) row i of the buffers
 *   belongs to state row d_rows[i]; unlisted rows keep their state bit for bit; d_count is then required.  A refused list changes no
 *   state and writes nothing except d_count->rows = -1.  Otherwise d_count (if given) = {n, 0, 0, 0}.
 *   Returns -1 with nothing enqueued: NULL v, d_pcm or d_sa_q8; d_rows without d_count; n outside (0, n_rows]; n_packets <= 0;
 *   packet_samples not a positive multiple of frame_samples or above 1920; n x P x packet_samples or n x P x F x 6 >= 2^31; d_pcm not
 *   16-byte aligned.  No allocation, no host synchronisation, one kernel (two with a list) on hip_stream: it can sit in a captured tick.
 * solo_vad_select: the stateful selection, room by room (room ids as in solo_mix: -1 = in no room -- nothing is written for such a row
 *   and its state does not move; an id outside [-1, n_rooms) is found on the device and refuses the call: d_count->rows = -1, nothing
 *   else written, no state changed; the same for a bad d_rows).  d_sa_q8 uint8 [n][P][frames] and d_level uint8 [n][P] (values above
 *   127 count as 127) are what solo_vad wrote.  The packets run in order; for every row i in a room, with state (t, h, s):
 *     a   = max over f of sa[i][p][f];   thr = t ? off_q8 : on_q8
 *     a >= thr:  t = 1, h = hang_packets, cand = 1;   otherwise:  t = 0, cand = (h > 0), h = max(h - 1, 0)
 *     key = cand ? (127 - level[i][p]) + (s ? stick : 0) : -1
 *   Per room, sel = the first max_speakers CANDIDATES in the total order: larger key, then s = 1 before s = 0, then smaller row position
 *   i; a row that is no candidate is never selected.  Then s = (i in sel), d_sel[i][p] = s, d_dominant[room][p] (or NULL) = the first
 *   row of the order, -1 when the room has no candidate.  After the last packet d_gain_out[i] (or NULL) = s ? max(gain_in[i], 0) : 0
 *   (d_gain_in NULL = 4096) and d_keep[i] (or NULL) = cand.  d_count = {rows in rooms, rooms with a member, selected (row, packet) pairs,
 *   changes of s from one packet to the next, the s a row brings into the call included}.  Only integers: the output is a pure function
 *   of inputs and state, and P packets in one call equal P calls of one packet.
 *   Returns -1 with nothing enqueued: NULL v, d_sa_q8, d_level, d_room, params, d_sel or d_count; n outside (0, n_rows]; n_packets or
 *   frames <= 0; n_rooms outside (0, n_rows]; n x P x frames or n_rooms x P >= 2^31; max_speakers outside 1 .. 64; not
 *   0 <= off_q8 <= on_q8 <= 255; hang_packets outside 0 .. 1000; stick outside 0 .. 127.  No allocation (the room plan's scratch is the
 *   object's, sized at create), no host synchronisation, five short kernels (six with a list) on hip_stream.
 * Calls on one object must be ordered (same stream, or events).  INTEGRATION.md section 2 has the tick. */
#define SOLO_VAD_STATE_BYTES 128
typedef struct solo_vad_obj solo_vad_t;
typedef struct { int32_t rows, rooms, selected, changes; } solo_vad_count_t;    /* 16 bytes; rows = -1: refused on the device */
typedef struct { int32_t max_speakers, on_q8, off_q8, hang_packets, stick; } solo_vad_select_params_t;
solo_vad_t *solo_vad_create(int32_t n_rows, int32_t frame_samples);
void solo_vad_destroy(solo_vad_t *v);
int32_t solo_vad_reset(solo_vad_t *v, void *hip_stream);
int32_t solo_vad_reset_rows(solo_vad_t *v, const int32_t *h_rows, int32_t n, void *hip_stream);
int32_t solo_vad_get_state(solo_vad_t *v, const int32_t *d_rows, int32_t n, uint8_t *d_blob, void *hip_stream);
int32_t solo_vad_set_state(solo_vad_t *v, const int32_t *d_rows, int32_t n, const uint8_t *d_blob, void *hip_stream);
int32_t solo_vad(solo_vad_t *v, const int32_t *d_rows, int32_t n, const int16_t *d_pcm, int32_t n_packets, int32_t packet_samples,
                 uint8_t *d_sa_q8, int32_t *d_detail, uint8_t *d_level, solo_vad_count_t *d_count, void *hip_stream);
int32_t solo_vad_select(solo_vad_t *v, const int32_t *d_rows, int32_t n, const uint8_t *d_sa_q8, const uint8_t *d_level,
                        int32_t n_packets, int32_t frames, const int32_t *d_room, int32_t n_rooms,
                        const solo_vad_select_params_t *params, const int16_t *d_gain_in, uint8_t *d_sel, int16_t *d_gain_out,
                        uint8_t *d_keep, int32_t *d_dominant, solo_vad_count_t *d_count, void *hip_stream);
/* Adaptive play-out delay control: the policy between the receive reports and the mixer -- when a stream starts, when its play-out
 * delay grows by a packet (a 1 -> 2 stretch) or shrinks by one (a 2 -> 1 shortening) -- decided on the device with a state record per
 * stream, and executed: after solo_playout_tick every listed stream has ONE packet of audio in the fixed row layout solo_vad / solo_mix*
 * read.  A solo_playout_t is an object of its own; row s belongs to stream s of the handle it is ticked with.  Integers only, a total
 * order everywhere: the output is a pure function of the arrivals.
 *   state      SOLO_PLAYOUT_STATE_BYTES = 128 bytes per row, 32 int32 words: 0 run, 1 held, 2 cum, 3 cool, 4 age, 5 late_prev (uint32),
 *              6 pos, 7 zero, 8 .. 23 the ring (32 int16 slots, slot j in half j & 1 of word 8 + j / 2, -32768 = none), 24 .. 31 zero; and
 *              one packet of PCM, int16 [packet_samples], the HELD packet.  Create and the two resets leave everything zero (not running).
 *   params     start_ready >= 1; max_span >= 0 (0 = off); window W in 1 .. 32; tolerate 0 .. 3; 0 <= lo <= hi <= 64; cooldown 0 .. 1000;
 *              cost_gate (<= 0 = off).  They are the call's, not the object's: a tick may bring other values than the one before.
 * The rule, per listed row and tick, from the row's solo_recv_report_t (tracking on, margin_min cleared by every tick) and depth D:
 *   not running:  ready >= start_ready, or max_span > 0 and span >= max_span: the row STARTS -- every ring slot none, run = 1,
 *              held = cum = cool = age = pos = 0, late_prev = late, action NORMAL.  Otherwise IDLE and the record does not move.
 *   running, first the observation (held and cum as the tick before left them):
 *              dl = late - late_prev (uint32), late_prev = late;
 *              dl > 0: s = -1;  else margin_min < D: s = min(max(margin_min + held, -1), 1000);  else none
 *              ring[pos] = s - cum (or none), pos = (pos + 1) mod 32, age = min(age + 1, W)
 *              q = the (tolerate + 1)-th smallest VALUE among the last `age` slots, undefined with fewer values; e = q + cum
 *   then the first of:   held: HELD, cool = max(cool - 1, 0)  |  max_span > 0 and span >= max_span: ACCEL_FORCED  |  cool > 0: NORMAL, cool -= 1
 *              |  e defined, e < lo, ready >= 1, max_span == 0 or span + 1 < max_span: STRETCH  |  age >= W, e defined, e > hi, ready >= 2: ACCEL
 *              |  NORMAL.
 *   (The ring holds the arrivals' timing relative to the NETWORK, s - cum, which a move of the play-out does not change: no move clears it.
 *   It always has 32 slots; W only says how far back the quantile looks.  |cum| saturates at 16000.)
 *   Execution (render), gated = cost_gate > 0 and the largest entry of the row's splice costs (solo_timescale's d_cost) > cost_gate:
 *     IDLE          L zeros, status 0                                     HELD   the held packet, held = 0, status 0
 *     NORMAL        the packet decoded
 *     STRETCH       1 decoded -> 2: the first is heard, the second held; held = 1, cum += 1, cool = cooldown
 *       _GATED      the decoded packet is heard as it is, nothing else changes
 *     ACCEL         2 decoded -> 1: heard; cum -= 1, cool = cooldown       ACCEL_FORCED  the same, never gated
 *       _GATED      decoded packet 0 is heard, packet 1 held; held = 1
 *   d_outcome holds SOLO_PLAYOUT_IDLE .. SOLO_PLAYOUT_ACCEL_FORCED; d_action the plan's codes 0 IDLE, 1 NORMAL, 2 HELD, 3 STRETCH, 4 ACCEL,
 *   5 ACCEL_FORCED.  d_status is the decoder's status of rows that decoded, 0 for the others.
 * solo_playout_plan: d_reports [n] (16-byte aligned) -> the first half of the state update, d_action [n], and three compacted lists in row
 *   order: d_one = the streams of the NORMAL and STRETCH rows, d_two = those of the ACCEL and ACCEL_FORCED rows (both strictly increasing:
 *   valid lists of solo_recv_decode_streams), d_stretch_pos = where each STRETCH row stands in d_one; all int32 [n], entries beyond the
 *   counts are not written.  d_count (16-byte aligned) = {n_one, n_two, n_stretch, n}.  d_rows: a DEVICE list (strictly increasing inside
 *   [0, n_rows), checked on the device ahead of the work: a refused list writes n_one = -1 and nothing else, no state moves), or NULL with
 *   n = n_rows; unlisted rows keep their records bit for bit.  The object remembers where the plan put each row: the render that follows
 *   must bring the same d_rows and n.
 * solo_playout_gather: rows d_stretch_pos[0 .. n_stretch) of d_pcm_one [n_one][L] -> d_out [n_stretch][L], the input of solo_timescale 1 -> 2.
 * solo_playout_render: the plan's d_action, the decode outputs of d_one (one packet: d_pcm_one [n_one][L], d_status_one) and d_two (two:
 *   d_pcm_two [n_two][2][L], d_status_two), the scaler's outputs d_ts_stretch [n_stretch][2][L] with d_cost_stretch [n_stretch][2 L / block]
 *   and d_ts_accel [n_two][L] with d_cost_accel [n_two][L / block] (block_samples = the scaler's block: samplerate / 200) -> d_heard
 *   int16 [n][L] (row i = listed row i, 16-byte aligned like every PCM pointer here), d_outcome / d_status int32 [n], the held store and
 *   held / cum / cool of the records; d_count (or NULL; 16-byte aligned) = rows per outcome, outcome[0] = -1 and nothing else for a refused
 *   list.  Buffers of empty lists may be NULL.  A row whose action points outside the buffers brought is rendered IDLE.
 *   plan is two short kernels (three with a list), render two (three); no allocation, no host synchronisation: each can be captured.
 * solo_playout_tick: the receive side of a bridge tick in one call -- solo_recv_report (records, margins cleared), plan, ONE host read of
 *   the 16-byte plan count (the tick's only synchronisation), solo_recv_decode_streams(d_one, 1) and (d_two, 2), gather, solo_timescale
 *   1 -> 2 and 2 -> 1 with their costs, render; calls whose list is empty are skipped, the intermediates live in the object (sized at
 *   create).  d_count = {plan, render}, 16-byte aligned.  Returns -1 with nothing enqueued: NULL po, b, params or output; a handle
 *   without a ring, with a ring shallower than 2, with tracking off, or whose stream count or packet samples differ from the object's; a
 *   packet that solo_timescale does not take; parameters out of range; n outside (0, n_rows]; d_streams = NULL with n != n_rows; d_heard
 *   or d_count not 16-byte aligned.  A list refused on the device ends the tick after the plan: d_count->plan.n_one = -1, nothing else
 *   written, no state, queue or play-out position moved.
 * solo_playout_create: NULL unless n_rows > 0 and packet_samples is a positive multiple of 8, at most 1920.  solo_playout_reset_rows takes
 *   a HOST list (1 .. n_rows indices inside [0, n_rows), none twice, else -1).  solo_playout_get_state / _set_state copy the listed rows'
 *   128 + 2 x packet_samples bytes (record, then held PCM) to / from d_blob (4-byte aligned); d_rows is a DEVICE list or NULL for rows
 *   0 .. n - 1; plain copies, an index outside [0, n_rows) moves nothing.  Calls on one object must be ordered.  INTEGRATION.md section 2. */
#define SOLO_PLAYOUT_STATE_BYTES 128
#define SOLO_PLAYOUT_IDLE 0
#define SOLO_PLAYOUT_NORMAL 1
#define SOLO_PLAYOUT_HELD 2
#define SOLO_PLAYOUT_STRETCH 3
#define SOLO_PLAYOUT_STRETCH_GATED 4
#define SOLO_PLAYOUT_ACCEL 5
#define SOLO_PLAYOUT_ACCEL_GATED 6
#define SOLO_PLAYOUT_ACCEL_FORCED 7
typedef struct solo_playout_obj solo_playout_t;
typedef struct { int32_t start_ready, max_span, window, tolerate, lo, hi, cooldown, cost_gate; } solo_playout_params_t;   /* 32 bytes */
typedef struct { int32_t n_one, n_two, n_stretch, listed; } solo_playout_plan_count_t;    /* 16 bytes; n_one = -1: list refused on the device */
typedef struct { int32_t idle, normal, held, stretch, stretch_gated, accel, accel_gated, accel_forced; } solo_playout_render_count_t;   /* 32 bytes */
typedef struct { solo_playout_plan_count_t plan; solo_playout_render_count_t render; } solo_playout_count_t;              /* 48 bytes */
solo_playout_t *solo_playout_create(int32_t n_rows, int32_t packet_samples);
void solo_playout_destroy(solo_playout_t *po);
int32_t solo_playout_reset(solo_playout_t *po, void *hip_stream);
int32_t solo_playout_reset_rows(solo_playout_t *po, const int32_t *h_rows, int32_t n, void *hip_stream);
int32_t solo_playout_get_state(solo_playout_t *po, const int32_t *d_rows, int32_t n, uint8_t *d_blob, void *hip_stream);
int32_t solo_playout_set_state(solo_playout_t *po, const int32_t *d_rows, int32_t n, const uint8_t *d_blob, void *hip_stream);
int32_t solo_playout_plan(solo_playout_t *po, const solo_recv_report_t *d_reports, const int32_t *d_rows, int32_t n, int32_t depth,
                          const solo_playout_params_t *params, int32_t *d_action, int32_t *d_one, int32_t *d_two, int32_t *d_stretch_pos,
                          solo_playout_plan_count_t *d_count, void *hip_stream);
int32_t solo_playout_gather(solo_playout_t *po, const int16_t *d_pcm_one, int32_t n_one, const int32_t *d_stretch_pos, int32_t n_stretch,
                            int16_t *d_out, void *hip_stream);
int32_t solo_playout_render(solo_playout_t *po, const int32_t *d_rows, int32_t n, const solo_playout_params_t *params, int32_t block_samples,
                            const int32_t *d_action, int32_t n_one, int32_t n_two, int32_t n_stretch, const int16_t *d_pcm_one,
                            const int32_t *d_status_one, const int16_t *d_pcm_two, const int32_t *d_status_two, const int16_t *d_ts_stretch,
                            const int32_t *d_cost_stretch, const int16_t *d_ts_accel, const int32_t *d_cost_accel, int16_t *d_heard,
                            int32_t *d_outcome, int32_t *d_status, solo_playout_render_count_t *d_count, void *hip_stream);
int32_t solo_playout_tick(solo_playout_t *po, solo_batch_t *b, const int32_t *d_streams, int32_t n, const solo_playout_params_t *params,
                          int16_t *d_heard, int32_t *d_outcome, int32_t *d_status, solo_playout_count_t *d_count, void *hip_stream);
/* Level control and peak limiter for decoded rows: the stage between solo_vad and the selection / the mix.  It brings every row's speech
 * to target_level -dBov with a slewed gain and keeps every output sample within +-ceiling, so that a caller 20 dB below another is no
 * longer 20 dB below in every mix and no longer loses solo_vad_select's order to the loud one.  A solo_agc_t is an object of its own,
 * like a solo_vad_t, with the same conventions: compact rows int16 [n][P][L], 16-byte aligned; d_rows a DEVICE list, strictly
 * increasing inside [0, n_rows), checked on the device ahead of the work, d_count then required, a refused list writes
 * d_count->rows = -1 and nothing else and moves no state, unlisted rows keep their record bit for bit; reset_rows takes a HOST list of
 * 1 .. n_rows indices inside [0, n_rows), none twice; get_state / set_state are plain copies of uint8 [n][64] (4-byte aligned), an
 * index outside the object moves nothing.  AGC state is not part of a migration blob: it moves with get_state / set_state.
 *   state      SOLO_AGC_STATE_BYTES = 64 bytes per row, 16 int32 words: 0 run, 1 spl_q8 (the smoothed speech level in -dBov, Q8),
 *              2 gain_q8 (the gain in dB, Q8, signed), 3 g_q16 (the linear gain at the last sample of the previous packet), 4 env_q15 (the
 *              limiter envelope at the end of the previous packet), 5 .. 15 zero (the stage never writes them).  Create and the resets
 *              leave {0, 0, 0, 65536, 32768, 0 ...}.  Values are clamped when a call reads them: gain_q8 to +-7680, g_q16 to
 *              [0, A[60]], env_q15 to [0, 32768], so no blob can index outside a table.
 *   L = packet_samples   a multiple of 32 with 256 <= L <= 1920
 *   d_level_in uint8 [n][P], what solo_vad wrote; NULL: the call computes the same RFC 6464 level from the input samples
 *   d_sa_q8    uint8 [n][P][frames], what solo_vad wrote; NULL: activity 255 everywhere, frames is ignored
 *   d_pcm_out  int16 [n][P][L]; d_pcm_out == d_pcm_in (in place) is allowed, any other overlap of the two ranges is refused
 *   d_level_out (uint8 [n][P]), d_gain_q8 (int16 [n][P]) and d_count may each be NULL, except d_count with a list
 * The rule, per row, packets in order.  All shifts are arithmetic; 64-bit products where noted.  Tables (tools/gen_agc_tables.py, exact
 * decimal arithmetic, rounded to nearest): A[i] = round(65536 * 10^((i - 30) / 20)), i = 0 .. 60; B[r] = round(65536 * 10^(r / 5120)),
 * r = 0 .. 255; lin(d), d in [-7680, 7680], d + 7680 = 256 i + r: (A[i] * B[r] + 32768) >> 16 in 64 bits.
 *   1  lv = min(level_in, 127); a = max over f of sa[f]; speech = a >= sa_on_q8 and lv <= gate_level
 *   2  only in speech packets: run == 0: spl = lv << 8, run = 1; otherwise spl += (((lv << 8) - spl) * alpha_q8) >> 8 (in 64 bits);
 *      want = clamp(spl - (target_level << 8), -(max_cut_db << 8), max_boost_db << 8); gain += clamp(want - gain, -slew_down_q8, slew_up_q8)
 *   3  g0 = g_q16, g1 = lin(gain), g_q16 = g1; g[s] = g0 + (((g1 - g0) * min(s + 1, 256)) >> 8);
 *      y0[s] = (x[s] * g[s] + 32768) >> 16 in 64 bits
 *   4  blocks of 32 samples, B = L / 32: pk_b = max |y0| over block b; a_b = 32768 if pk_b <= ceiling, else floor(ceiling * 32768 / pk_b);
 *      a'_b = min(a_b, a_{b+1}) for b < B - 1, a'_{B-1} = a_{B-1} (one block of look-ahead inside the packet);
 *      e_{-1} = min(env_q15, a_0); e_b = min(a'_b, e_{b-1} + release_q15); env_q15 = e_{B-1}
 *   5  s = 32 b + t: env[s] = e_{b-1} + (((e_b - e_{b-1}) * (t + 1)) >> 5); y[s] = (y0[s] * env[s] + 16384) >> 15 in 64 bits.
 *      Both ends of the interpolation are <= a_b, so |y[s]| <= ceiling for every sample: there is no saturation step.
 *   6  d_level_out = the RFC 6464 level of y from its exact energy (as solo_vad's); d_gain_q8 = gain after the packet;
 *      d_count = {rows processed, (row, packet) pairs with speech, pairs with some e_b < 32768, 0}
 * The limiter does not see the next packet: one that opens louder than the last one closed steps the envelope down to a_0 at the
 * boundary.  P packets in one call equal P calls of one packet.
 * Returns -1 with nothing enqueued: NULL g, d_pcm_in, d_pcm_out or params; n outside (0, n_rows]; d_rows without d_count;
 * n_packets <= 0; L not as above; d_sa_q8 with frames <= 0; n x P x L or n x P x frames >= 2^31; PCM not 16-byte aligned; the PCM
 * ranges overlapping in part; target_level or gate_level outside 0 .. 127; max_boost_db or max_cut_db outside 0 .. 30; sa_on_q8 outside
 * 0 .. 255; alpha_q8 outside 1 .. 256; slew_up_q8 or slew_down_q8 outside 0 .. 7680; ceiling outside 1 .. 32767; release_q15 outside
 * 0 .. 32768.  No allocation, no host synchronisation, one kernel (two with a list) on hip_stream: it can sit in a captured tick.
 * Calls on one object must be ordered (same stream, or events).  INTEGRATION.md section 2 has the tick. */
#define SOLO_AGC_STATE_BYTES 64
typedef struct solo_agc_obj solo_agc_t;
typedef struct { int32_t target_level, max_boost_db, max_cut_db, sa_on_q8, gate_level, alpha_q8,
                 slew_up_q8, slew_down_q8, ceiling, release_q15; } solo_agc_params_t;      /* 40 bytes */
typedef struct { int32_t rows, speech, limited, zero; } solo_agc_count_t;                  /* 16 bytes; rows = -1: list refused */
solo_agc_t *solo_agc_create(int32_t n_rows);
void    solo_agc_destroy(solo_agc_t *g);
int32_t solo_agc_reset(solo_agc_t *g, void *hip_stream);
int32_t solo_agc_reset_rows(solo_agc_t *g, const int32_t *h_rows, int32_t n, void *hip_stream);
int32_t solo_agc_get_state(solo_agc_t *g, const int32_t *d_rows, int32_t n, uint8_t *d_blob, void *hip_stream);
int32_t solo_agc_set_state(solo_agc_t *g, const int32_t *d_rows, int32_t n, const uint8_t *d_blob, void *hip_stream);
int32_t solo_agc(solo_agc_t *g, const int32_t *d_rows, int32_t n, const int16_t *d_pcm_in, int32_t n_packets, int32_t packet_samples,
                 const uint8_t *d_level_in, const uint8_t *d_sa_q8, int32_t frames, const solo_agc_params_t *params,
                 int16_t *d_pcm_out, uint8_t *d_level_out, int16_t *d_gain_q8, solo_agc_count_t *d_count, void *hip_stream);
/* Stream migration: the state of a running call leaves a handle as a DEVICE blob and enters any slot of any handle of the same
 * geometry -- on this GPU, or on another one after the caller has moved the bytes (the blob is plain device memory: a torch.distributed
 * send, a hipMemcpyPeer).  The call goes on where it stood: no first-frame logic, no cold-start concealment, VAD / DTX / CNG / PLC and
 * gain histories intact.  For draining a GPU, rebalancing ranks, gathering a room's participants in one handle (solo_mix), standby copies.
 *   which      1 = encoder state, 2 = decoder state, 4 = receive queue (payload, length words, play-out position, the per-stream
 *              counters of solo_recv_track), or a sum of them
 *   d_streams  int32 [n], DEVICE list as in the subset calls: strictly increasing inside [0, N), checked on the device
 *   d_blob     uint8 [n][blob_stride]: row i belongs to d_streams[i]; 16-byte aligned, blob_stride a multiple of 16 and
 *              >= solo_batch_state_bytes(b, which)
 *   d_count    one solo_migrate_count_t on the device
 * Record: a 64-byte header (magic, version, the sections present, the geometry of each -- samplerate, frames per packet, joint mode,
 * the size of the stream record; ring depth and slot_bytes --, the origin stream, the body length, two checksums over the body's
 * 32-bit words: sum w_i and sum (i + 1) w_i mod 2^32), then the sections in bit order, each padded to 16 bytes.  Sections 1 and 2 are the
 * stream's records byte for byte, rate / DTX / useMDIndex included.  Section 4 is written in play-relative order (entry k = sequence
 * number play + k) and only the bytes its length words declare, the rest zero: equal queues give equal blobs wherever the ring's
 * storage wraps.  solo_amd/csrc/solo_migrate.h has the layout word by word.
 * A BLOB IS VALID ONLY FOR THE LIBRARY BUILD THAT WROTE IT (the size words enforce it): a migration and standby format, not an archive.
 * solo_batch_state_bytes: bytes of one record, header included, a multiple of 16; -1 when which is 0, has unknown bits or names a
 *   direction or a ring the handle lacks.
 * Both calls return -1 with nothing enqueued for a NULL pointer, n outside (0, N], such a `which`, a stride below
 *   solo_batch_state_bytes(b, which), a stride or a base that is not 16-byte aligned.
 * solo_batch_export_streams reads only: every state, queue and play-out position stays bit for bit.  d_count = {n, 0, bytes written};
 *   a refused list writes d_count->streams = -1 and nothing else.
 * solo_batch_import_streams checks EVERY record before it copies anything; the call is refused as a whole, d_count = {-1, index of the
 *   first bad record + 1, 0}, when the list is invalid (the bad position counts as the record), or a record has a wrong magic or
 *   version, lacks a section of `which`, differs from the handle in samplerate, frames per packet, joint mode, record size or (section 4)
 *   ring depth / slot_bytes, has a wrong body length, a wrong checksum, or queue words no ring could hold.  After a refused import every
 *   state of the handle is bit for bit what it was.  Otherwise the listed streams hold exactly the imported state -- their own rate, DTX and
 *   useMDIndex included, whatever control the handle was created with (as after solo_batch_reset_streams) --, unlisted streams are
 *   untouched and d_count = {n, 0, bytes taken}.  A blob may hold more sections than the call takes.  With section 4 the queue of a listed
 *   stream is replaced entirely; the handle-wide solo_recv_stats words do not change; the per-stream counters are written only if the
 *   handle has allocated them (solo_recv_track(b, 1) at any time before).
 * Ordering as solo_batch_reset_streams: the kernels wait for this handle's encode work still in flight on its internal streams
 * (async joins included) and for its latest decode call, whichever stream that was issued on; work enqueued on hip_stream after the call sees the result.  No host synchronisation, no allocation.  The words
 * of the persistent encoder schedule (flags, tickets) belong to the handle and do not travel: an imported stream encodes under the
 * default schedule like any other.  The legacy AGR_Sate_* handles are not covered. */
typedef struct { int32_t streams, refused; int64_t bytes; } solo_migrate_count_t;   /* 16 bytes */
int64_t solo_batch_state_bytes(const solo_batch_t *b, int32_t which);
int32_t solo_batch_export_streams(solo_batch_t *b, const int32_t *d_streams, int32_t n, int32_t which,
                                  uint8_t *d_blob, int64_t blob_stride, solo_migrate_count_t *d_count, void *hip_stream);
int32_t solo_batch_import_streams(solo_batch_t *b, const int32_t *d_streams, int32_t n, int32_t which,
                                  const uint8_t *d_blob, int64_t blob_stride, solo_migrate_count_t *d_count, void *hip_stream);
/* RTP at both ends of the bridge: solo_rtp_pack puts an RTP header (RFC 3550 section 5.1) in front of every datagram solo_send_pack /
 * solo_send_fanout recorded, so that what leaves the device is what the socket sends; solo_rtp_parse turns received datagrams into the
 * arrivals solo_recv_insert takes, in place (no payload byte moves twice).  The RFC 6464 audio level of solo_vad / solo_agc travels in a
 * one-byte header extension (RFC 8285 section 4.2) and is read back without decoding.  A solo_rtp_t is an object of its own beside a
 * handle: the per-stream configuration and a sorted (SSRC, stream) table on the device, a mirror of both on the host.  The device code
 * never writes them: with the configuration held fixed, both calls are pure functions of their inputs.
 *   packet_samples   timestamp ticks per packet: 320, 640 or 1280 (the handle's packet samples)
 * Control plane -- HOST arrays, as for solo_batch_reset_streams.  solo_rtp_bind gives the listed streams their SSRC, timestamp offset,
 * sequence offset (the random starts of RFC 3550) and the payload types of MD1 and of MD2 || HB (0 .. 127; equal types: the receiver reads
 * the description from the payload, which takes useMDIndex = 1) and marks them bound; level_id, the RFC 8285 element id of the audio
 * level (1 .. 14; 0: parse looks for none, pack takes no levels), belongs to the session: the latest bind wins.  solo_rtp_unbind takes
 * the binding away (a stream that has none stays so).  Both rebuild the table from the mirror, are ordered on hip_stream, return when
 * the table is on the device and are not capturable; a captured pack or parse reads the configuration of the moment it runs.  -1, and
 * nothing changes: NULL r or array; n <= 0; an index outside [0, n_streams) or listed twice; a payload type above 127; level_id outside
 * 0 .. 14; an SSRC that two bound streams would share after the call.  The host mirror moves only after the device holds the call's
 * records and table: a call whose launches or copy fail is judged afterwards against what the session held before it.
 * Wire format: 12 bytes, V = 2, P = 0, CC = 0, M = 0; PT = pt_md1 for description 0, pt_md2 for description 1; sequence number =
 * seq_offset + 2 seq + desc mod 2^16 (a description that is not sent shows as a gap); timestamp = ts_offset + seq x packet_samples mod
 * 2^32; the stream's SSRC.  With levels X = 1 and 8 more bytes: 0xBE 0xDE 0x00 0x01, level_id << 4, the level byte as it is (V << 7 |
 * level), two zero bytes.  Header and payload are contiguous; every datagram starts at a multiple of 4 of d_wire and the 0 .. 3 bytes
 * behind it are written as zero.
 * solo_rtp_pack
 *   d_records, d_send_count   what solo_send_pack / solo_send_fanout wrote; the records of the call are min(d_send_count->records,
 *                    max_records), READ ON THE DEVICE: the call can sit behind solo_send_pack in one captured graph.
 *                    d_send_count->records < 0 (a refused list): d_count->dgrams = -1 and nothing else is written
 *   d_payload        the pool the records point into, payload_bytes long; offsets may repeat (fanout)
 *   d_level          uint8 [n_streams][level_depth] or NULL (no extension): the byte of packet seq of stream s is
 *                    d_level[s x level_depth + seq % level_depth]
 *   d_dgrams         solo_dgram_t [max_records]: entry k belongs to record k (packet-major order is kept): where its datagram lies in d_wire,
 *                    header included; {0, 0} for a record that is refused or cut by the cap.  Entries behind the call's records stay
 *   d_wire           uint8 [wire_capacity]: the offsets are the running sum of roundup4(H + len) over the valid records, H = 12 or 20
 *   d_count          one solo_rtp_pack_count_t (8-byte aligned): written and needed datagrams and bytes (pad bytes included), refused records
 * Record k is refused -- and its payload never read -- when its stream is outside [0, n_streams) or not bound, desc is not 0 or 1, seq < 0,
 * len <= 0, len > 32767 or [offset, offset + len) is not inside the pool.  A datagram is written iff it and its pad bytes end inside
 * min(wire_capacity, 2^31 - 1): what is written is a prefix, nothing is written at or beyond the cap, wire_capacity = 0 only counts;
 * d_count->bytes_needed is the capacity that never overflows.
 * -1 with nothing enqueued: a NULL pointer other than d_level; max_records <= 0; a negative payload_bytes or wire_capacity; d_level with
 * level_depth <= 0 or while the session's level_id is 0; d_records, d_send_count, d_dgrams or d_wire not 4-byte, d_count not 8-byte
 * aligned.  Three short kernels on hip_stream only, no host synchronisation; the session's scratch for the scan (16 bytes per 256
 * records) grows, with a stream synchronisation, when max_records is larger than in every call before.
 * solo_rtp_parse
 *   b                the receiving handle: it must have a receiver ring, the session's stream count and packet samples (-1 otherwise)
 *   d_dgrams, d_wire n_dgrams datagrams inside d_wire (wire_bytes long), at any byte alignment
 *   d_arrivals       solo_arrival_t [n_dgrams]: arrival i belongs to datagram i, its offset points at the payload inside d_wire -- then
 *                    solo_recv_insert(b, d_arrivals, n_dgrams, d_wire, wire_bytes, hip_stream).  A rejected datagram yields
 *                    {stream = -1, 0, 0, 0, 0}, WHICH THE RING COUNTS AS `bad`: d_count, not the ring's statistics, says why
 *   d_level_out      uint8 [n_dgrams] or NULL: the level byte of an accepted datagram with X set, profile 0xBEDE and level_id > 0 -- the
 *                    first one-byte element with id level_id and one data byte (id 0: a pad byte; id 15, or an element that reaches over
 *                    the block's end: the walk stops); 255: none, any other profile (the two-byte form included) and rejected datagrams
 *                    (a sender's byte 255, "voice at -127 dBov", therefore reads as none)
 *   d_rtp_seq_out    uint16 [n_dgrams] or NULL: the raw 16-bit sequence number (0 for a rejected datagram), for transport statistics
 *   d_count          one solo_rtp_parse_count_t: a counter per verdict
 * The verdict is the FIRST rule that fails: malformed (len < 12 or a range outside [0, min(wire_bytes, 2^31 - 1)); 12 + 4 CC or the
 * extension block, 4 + 4 x length with X set, reaches past the datagram; P set with a pad count of 0 or larger than what is left; no
 * payload byte left; more than 32767 payload bytes), version (V != 2), unknown_ssrc (binary search of the bound table), unknown_pt
 * (neither of the stream's two; equal types give desc = -1), timestamp.  The packet number comes from the TIMESTAMP, not from the
 * sequence number, so any sender that stamps both descriptions with the packet's sampling instant interoperates; it is unwrapped against
 * the stream's play-out position p (the ring's, read on the device): delta = (int32)(ts - ts_offset - (uint32)p x L) must be a multiple
 * of L, seq = p + delta / L must lie in 0 .. 2^31 - 1.  No state, no dependence on arrival order, a window of about +-3.3 M packets at
 * L = 640; late and ahead stay the ring's decision.
 * -1 with nothing enqueued: NULL r, b or d_count; b as above; n_dgrams < 0 or wire_bytes < 0; with n_dgrams > 0 a NULL d_dgrams, d_wire or
 * d_arrivals; d_dgrams, d_arrivals or d_count not 4-byte, d_rtp_seq_out not 2-byte aligned.  Two kernels (the clear of the count, then a lane per
 * datagram) on hip_stream, no allocation, no host synchronisation: capturable with n_dgrams frozen.  Calls on a handle must be ordered
 * with the rest of the ring (same stream, or events).  INTEGRATION.md section 2 has the tick. */
typedef struct solo_rtp_obj solo_rtp_t;
typedef struct { int32_t offset, len; } solo_dgram_t;      /* 8 bytes: one datagram inside a wire buffer */
typedef struct {
    int32_t dgrams, dgrams_needed;     /* written / what the call would have written without the cap; dgrams = -1: refused list */
    int64_t bytes, bytes_needed;       /* the same for wire bytes, pad bytes included */
    int32_t refused, reserved;         /* records that yield no datagram; 0 */
} solo_rtp_pack_count_t;               /* 32 bytes */
typedef struct { int32_t accepted, with_level, malformed, version, unknown_ssrc, unknown_pt, timestamp, reserved; } solo_rtp_parse_count_t;   /* 32 bytes */
/* The session's lifecycle and control plane, then its two device calls. */
solo_rtp_t *solo_rtp_create(int32_t n_streams, int32_t packet_samples);
void    solo_rtp_destroy(solo_rtp_t *r);
int32_t solo_rtp_bind(solo_rtp_t *r, const int32_t *h_streams, int32_t n, const uint32_t *h_ssrc, const uint32_t *h_ts_offset,
                      const uint16_t *h_seq_offset, const uint8_t *h_pt_md1, const uint8_t *h_pt_md2, int32_t level_id, void *hip_stream);
int32_t solo_rtp_unbind(solo_rtp_t *r, const int32_t *h_streams, int32_t n, void *hip_stream);
int32_t solo_rtp_pack(solo_rtp_t *r, const solo_arrival_t *d_records, const solo_send_count_t *d_send_count, int32_t max_records,
                      const uint8_t *d_payload, int64_t payload_bytes, const uint8_t *d_level, int32_t level_depth,
                      solo_dgram_t *d_dgrams, uint8_t *d_wire, int64_t wire_capacity, solo_rtp_pack_count_t *d_count, void *hip_stream);
int32_t solo_rtp_parse(solo_rtp_t *r, solo_batch_t *b, const solo_dgram_t *d_dgrams, int32_t n_dgrams, const uint8_t *d_wire, int64_t wire_bytes,
                       solo_arrival_t *d_arrivals, uint8_t *d_level_out, uint16_t *d_rtp_seq_out, solo_rtp_parse_count_t *d_count,
                       void *hip_stream);
/* SRTP at both ends (RFC 3711, the mandatory default transforms): solo_srtp_protect stands behind solo_rtp_pack and turns the packed
 * datagrams into SRTP in place, solo_srtp_unprotect stands in front of solo_rtp_parse and turns received SRTP datagrams back into RTP in
 * place, so that a secured deployment walks no datagram on the host either.  Cipher AES-128 in counter mode (AES_CM_128) over everything
 * behind the RTP header (12 + 4 CC bytes and the extension block: the RFC 6464 level stays readable for a forwarding server),
 * authentication HMAC-SHA1 over header, ciphertext and rollover counter with an 80- or 32-bit tag (HMAC_SHA1_80 / _32), key derivation
 * of section 4.3 with rate 0.  The keys belong to the solo_rtp_t session, which already has the SSRC table and the sequence offsets.
 * solo_rtp_set_trailer -- a host switch, 0 .. 16, default 0, read when a pack call is issued: with a trailer T solo_rtp_pack plans every
 *   valid record as roundup4(H + len + T), writes the T bytes behind the datagram as zero together with the pad bytes, leaves
 *   d_dgrams[k].len = H + len, counts the trailer in bytes and bytes_needed, and writes a datagram iff all of it fits the cap.  T = 0:
 *   every byte and count as without the call.  -1: NULL r, a value outside 0 .. 16, or one below the tag of a stream's tx key.
 * Control plane -- HOST arrays, as for solo_rtp_bind; ordered on hip_stream, the calls return when the device holds the records, not
 * capturable.  The device holds per stream and direction a 256-byte record: the expanded AES round keys, the salt at its place in the
 * IV, the SHA-1 states behind the HMAC's ipad and opad blocks, the tag length and a "has key" word, derived ON THE HOST from one
 * direction's SDES / DTLS-SRTP keying material (master key || master salt) with labels 0, 1, 2 and index 0; and per stream a receive
 * record, the highest authenticated packet index.  The records are a device allocation made by the first solo_srtp_set_keys: a session
 * without SRTP pays nothing.  The host keeps per stream "has tx / has rx / tag bytes" and never the keys; it moves after the device does.
 *   solo_srtp_set_keys    h_tx_master / h_rx_master: [n][30] or NULL = that direction keeps what it had; h_rx_roc: [n] initial rollover
 *                    counters or NULL = 0; a call that sets a stream's rx key resets its receive record to "none yet" with that counter.
 *                    -1, nothing changed: NULL r or list; n <= 0, an index outside [0, n_streams) or listed twice; tag_bytes other
 *                    than 4 or 10; both masters NULL; a tx key while the session's trailer is smaller than tag_bytes
 *   solo_srtp_clear_keys  both keys and the receive record of the listed streams go (zeroed on the device).  solo_rtp_unbind does the
 *                    same for its streams: a slot taken by the next call never inherits them; solo_rtp_destroy zeroes all records
 *   solo_srtp_get_rx_index  h_index[i] = the highest authenticated index (ROC << 16 | SEQ) of listed stream i, -1: none yet.  With
 *                    solo_srtp_set_keys' h_rx_roc this is the hand-over of a receiver to another session
 * solo_srtp_protect -- datagram k belongs to record k; the records of the call are min(d_send_count->records, max_records), read on the
 *   device as in pack; d_send_count->records < 0: d_count->ok = -1, no datagram is touched.  d_dgrams[k].len == 0 (refused by pack, or
 *   cut): skipped.  The stream has no tx key: d_dgrams[k] becomes {0, 0}, counted no_key -- NOTHING OF A SESSION'S LEAVES IN THE CLEAR
 *   THROUGH THIS CALL.  Otherwise the packet index is i = seq_offset + 2 seq + desc, the unreduced integer behind pack's sequence number,
 *   ROC = (i >> 16) mod 2^32 (the sender keeps no state: protect is a pure function like pack); IV = (k_s << 16) ^ (SSRC << 64) ^
 *   (i << 16); keystream block j = AES(k_e, IV + j), XORed over the bytes behind the header; tag = the first tag_bytes of
 *   HMAC-SHA1(k_a, header || ciphertext || ROC as 4 big-endian bytes), written at [len, len + tag_bytes): pack's trailer is its room;
 *   d_dgrams[k].len += tag_bytes.  malformed, voided like no_key: a datagram whose range or tag reaches past wire_bytes, shorter than 12
 *   bytes or whose header reaches past its end, or a record whose stream, seq or desc pack would refuse.
 *   -1 with nothing enqueued: a NULL pointer; max_records <= 0; wire_bytes < 0; d_records, d_send_count, d_dgrams or d_count not 4-byte
 *   aligned.  Two kernels (the clear of the count, a workgroup per 256 datagrams) on hip_stream, no allocation, no host synchronisation:
 *   capturable with max_records frozen.
 * solo_srtp_unprotect -- n_dgrams datagrams inside d_wire at any byte alignment, their ranges disjoint.  The verdict is the FIRST rule that
 *   fails: malformed (a range outside [0, min(wire_bytes, 2^31 - 1)); len < 12 + tag; 12 + 4 CC or the extension block reaching past
 *   len - tag; tag = that of the stream's rx key, and 4 where the SSRC or the key is not known), unknown_ssrc (the table search of
 *   parse), no_key, auth_failed.  AUTHENTICATE FIRST: only an accepted datagram is decrypted, d_dgrams_out[i] = {offset, len - tag},
 *   ready for solo_rtp_parse (d_dgrams_out may be d_dgrams); a rejected datagram leaves every wire byte as it was and yields {0, 0},
 *   which parse counts as malformed and the ring as bad.  The rollover counter is estimated by RFC 3711 section 3.3.1 / appendix A
 *   against the stream's receive record as it stood when the call began (none yet: the initial counter; s_l < 32768: ROC - 1 when
 *   SEQ - s_l > 32768; s_l >= 32768: ROC + 1 when s_l - 32768 > SEQ), index = v << 16 | SEQ; behind the verdicts a second short kernel
 *   raises each stream's record to the highest index the call accepted.  The result does not depend on the order inside the call and
 *   equals the RFC's packet-by-packet receiver unless one call holds datagrams of a stream more than 2^15 sequence numbers apart.
 *   THERE IS NO REPLAY LIST: a replayed datagram reaches the ring, which drops it as duplicate or late.
 *   -1 with nothing enqueued: NULL r or d_count; n_dgrams < 0 or wire_bytes < 0; with n_dgrams > 0 a NULL d_dgrams, d_wire or
 *   d_dgrams_out; d_dgrams, d_dgrams_out or d_count not 4-byte aligned.  Three kernels on hip_stream, no allocation, no host
 *   synchronisation: capturable with n_dgrams frozen.  Not built: MKI, RFC 6904, AES-256. */
#define SOLO_SRTP_MASTER_BYTES 30   /* master key (16) || master salt (14): one direction's SDES / DTLS-SRTP keying material */
typedef struct { int32_t ok, skipped, malformed, unknown_ssrc, no_key, auth_failed, reserved[2]; } solo_srtp_count_t;   /* 32 bytes */
/* The trailer switch and the key calls of the session, then its two SRTP device calls. */
int32_t solo_rtp_set_trailer(solo_rtp_t *r, int32_t trailer_bytes);
int32_t solo_srtp_set_keys(solo_rtp_t *r, const int32_t *h_streams, int32_t n, const uint8_t *h_tx_master, const uint8_t *h_rx_master,
                           const uint32_t *h_rx_roc, int32_t tag_bytes, void *hip_stream);
int32_t solo_srtp_clear_keys(solo_rtp_t *r, const int32_t *h_streams, int32_t n, void *hip_stream);
int32_t solo_srtp_get_rx_index(solo_rtp_t *r, const int32_t *h_streams, int32_t n, int64_t *h_index, void *hip_stream);
int32_t solo_srtp_protect(solo_rtp_t *r, const solo_arrival_t *d_records, const solo_send_count_t *d_send_count, int32_t max_records,
                          solo_dgram_t *d_dgrams, uint8_t *d_wire, int64_t wire_bytes, solo_srtp_count_t *d_count, void *hip_stream);
int32_t solo_srtp_unprotect(solo_rtp_t *r, const solo_dgram_t *d_dgrams, int32_t n_dgrams, uint8_t *d_wire, int64_t wire_bytes,
                            solo_dgram_t *d_dgrams_out, solo_srtp_count_t *d_count, void *hip_stream);
/* Forwarding without transcoding: the middle of a forwarding server's tick.  Such a server reads its senders' RFC 6464 levels without
 * decoding and copies a selected sender to the other members of its room; it has neither decoder nor encoder.  solo_forward_levels turns
 * the arrivals solo_rtp_parse wrote into one level per row, which solo_vad_select takes; solo_forward_route turns the selected speakers'
 * arrivals into records for solo_rtp_pack, under per-room slots whose packet numbers stay continuous when the speaker behind a slot
 * changes.  No payload byte moves: a record's offset and len are the arrival's own and point into the receive buffer, which the egress
 * solo_rtp_pack is given as its pool.
 * The wire model: a room has K slots (K = slots, 1 .. 8, normally the max_speakers given to solo_vad_select); a selected speaker holds one
 * slot of its room for as long as it stays selected.  Every row m of the room receives slot k as egress stream m x K + k, a stream of a
 * second solo_rtp_t of n_rows x K streams that the caller binds with SSRCs of its own (distinct payload types: the records carry desc
 * 0 / 1) and, for SRTP, the receivers' keys.  A row does not receive the slot it holds itself.  solo_rtp_pack derives sequence number and
 * timestamp from the record's packet number, so a slot stays continuous across a change of speaker if the packet number does: that
 * number is the state this object keeps, 16 bytes {int32 src, delta, start, next} per room and slot.
 * Object and control plane -- a row-state object like solo_vad_t whose "row" is a ROOM.  solo_forward_create: NULL for n_rows <= 0 or
 * slots outside 1 .. 8.  solo_forward_reset: every room; solo_forward_reset_rooms: a HOST list, -1 for an index outside [0, n_rows) or
 * listed twice; a reset leaves {src = -1, delta = 0, start = 0, next = 0} in every slot.  solo_forward_get_state / _set_state: a DEVICE
 * list of rooms or NULL, uint8 [n][16 x K], as the other row objects.  Lifecycle and state calls come before a capture.
 * solo_forward_levels -- stateless, needs no object.  An arrival COUNTS when its stream is inside [0, n_rows) and its desc is 0 or 1 (a
 *   rejected datagram, stream = -1, does not; nor does desc = -1, a sender bound with equal payload types: solo_rtp_pack takes only
 *   0 / 1).  The byte of a counting arrival i is d_level_in[i] unless that is 255, otherwise default_level unless that is 255 too (255:
 *   the datagram has no byte); d_level_in NULL: every datagram has default_level.  For row s, over its counting arrivals, d_rowinfo[s] =
 *   {min_seq, max_seq: the smallest and largest seq, -1, -1 if there is none (an arrival's seq is 0 .. 2^31 - 1); dgrams: their number;
 *   byte: the byte with the smallest key (byte & 127) << 1 | !(byte >> 7), i.e. the loudest, voiced before unvoiced at equal level, 0x7F
 *   if no arrival has a byte; level = byte & 127; sa = 255 if byte & 128, else 0; pad = 0}.  d_sa_q8[s] and d_level[s] (uint8 [n_rows])
 *   receive sa and level: what solo_vad_select takes with n_packets = 1, frames = 1.  Every row is written; the result is a pure
 *   function of the inputs and independent of the order of the arrivals.
 *   -1 with nothing enqueued: a NULL output; n_dgrams < 0, or n_dgrams > 0 with NULL d_arrivals; n_rows <= 0; default_level outside
 *   0 .. 255; d_rowinfo or d_arrivals not 4-byte aligned.  Three short kernels (a clear, a lane per datagram with atomic min / max / add
 *   on the row's words, a lane per row that turns the winning key into the bytes) on hip_stream, no allocation, no host synchronisation:
 *   capturable with n_dgrams frozen (tests/test_gpu_forward.py: test_capture_forward_tick).
 * solo_forward_route -- d_sel: uint8 [n] as solo_vad_select wrote it for one packet; d_room: the ids of solo_mix, -1 = in no room, the
 *   members of room r are the rows i < n with d_room[i] == r.
 *   Step 1, slots, per room r in this order: a slot whose src is a row x with x < n, d_room[x] == r and d_sel[x] != 0 keeps it, every
 *   other slot becomes free (src = -1; start, next and delta stay).  The selected members of r that hold no slot AND have
 *   d_rowinfo[x].dgrams > 0 take the free slots, in increasing row order, lowest free k first; a slot that takes row x gets src = x,
 *   start = next, delta = next - d_rowinfo[x].min_seq, and adds 1 to `switches`.  Members left over when the slots run out hold none this
 *   call; a selected member with no datagram this call takes no slot yet.
 *   Step 2, the verdict of arrival i, the FIRST rule that fails, each with a counter: rejected (stream outside [0, n)), no_desc (desc not
 *   0 / 1), no_room (the sender's room is -1), not_selected (d_sel[sender] == 0), no_slot (the sender holds no slot after step 1), stale
 *   (q = seq + delta, computed in 64 bits, is outside [start, 2^31 - 2]); otherwise the arrival is forwarded.
 *   Step 3, records: a forwarded arrival of sender s in slot k of room r yields one record per member m != s of r, in increasing m:
 *   {stream = m x K + k, seq = q, desc, offset, len}, offset and len the arrival's own.  The records are ordered by arrival index, then
 *   by m; record j is written iff j < max_records, so what is written is a prefix and max_records = 0 only counts.  d_send_count has the
 *   form solo_rtp_pack and solo_srtp_protect read on the device: records / records_needed = written / needed, bytes / bytes_needed = the
 *   sum of len over the same two sets, empty = refused = 0.  A DUPLICATE DATAGRAM IS FORWARDED TWICE: there is no ring here, the
 *   receivers' rings drop it.
 *   Step 4, after the records: for every slot with a source, next = max(next, d_rowinfo[src].max_seq + delta + 1), taken only if that
 *   value is within [start + 1, 2^31 - 1].  d_level_fwd (uint8 [n x K], or NULL) receives, for every row m in a room and every k,
 *   d_rowinfo[src].byte of its room's slot k, or 0x7F for a free slot (rows in no room are not written): d_level of the egress
 *   solo_rtp_pack with level_depth = 1.  d_slot_src (int32 [n_rooms][K], or NULL) receives src of every slot: the signalling plane tells
 *   receivers from it who a slot carries.
 *   Refusal on the device: a room id outside [-1, n_rooms) is found ahead of everything else; then d_count->forwarded = -1,
 *   d_send_count->records = -1 (the egress pack and protect then write nothing), and no state, record or other output is touched.
 *   -1 with nothing enqueued: NULL f, d_rowinfo, d_sel, d_room, d_records, d_send_count or d_count; n or n_rooms outside (0, n_rows];
 *   n_dgrams < 0, or n_dgrams > 0 with NULL d_arrivals; max_records < 0; n_dgrams x (n - 1) >= 2^31; d_arrivals, d_rowinfo, d_room,
 *   d_records, d_slot_src or d_count not 4-byte, d_send_count not 8-byte aligned.
 *   Every output and the state after the call are a pure function of inputs and state, independent of the order of the arrivals except
 *   for the order of the records, which follows the arrivals by definition.  Nine short kernels on hip_stream (the room plan's four, the
 *   counts, a wavefront per room, a lane per arrival, a scan, a lane per OUTPUT record), no host synchronisation.  What depends on n_rows
 *   belongs to the object and is sized at create; the scratch for the scan over the arrivals (12 bytes per datagram) grows, with a stream
 *   synchronisation, only when a call has more datagrams than every one before it: capturable with n_dgrams, n and max_records frozen
 *   (tests/test_gpu_forward.py: test_capture_forward_tick).  Calls on one object must be ordered (same stream, or events).
 * A row that changes room while it holds a slot loses the slot in its old room and takes a free one in the new room like any newcomer.
 * A room id that is used again for another conference keeps its slots' packet numbers unless solo_forward_reset_rooms is called (and the
 * egress streams rebound).  A receiver that joins mid-call: its slot streams simply begin.  INTEGRATION.md section 2 has the tick. */
typedef struct solo_forward_obj solo_forward_t;
typedef struct { int32_t min_seq, max_seq, dgrams; uint8_t sa, level, byte, pad; } solo_forward_row_t;      /* 16 bytes */
typedef struct { int32_t forwarded, rejected, no_desc, no_room, not_selected, no_slot, stale, switches; } solo_forward_count_t;  /* 32 bytes; forwarded = -1: refused on the device */
#define SOLO_FORWARD_STATE_BYTES(slots) (16 * (slots))   /* per room: {int32 src, delta, start, next} per slot */
/* The object's lifecycle and control plane, then the two device calls. */
solo_forward_t *solo_forward_create(int32_t n_rows, int32_t slots);
void    solo_forward_destroy(solo_forward_t *f);
int32_t solo_forward_reset(solo_forward_t *f, void *hip_stream);
int32_t solo_forward_reset_rooms(solo_forward_t *f, const int32_t *h_rooms, int32_t n, void *hip_stream);
int32_t solo_forward_get_state(solo_forward_t *f, const int32_t *d_rooms, int32_t n, uint8_t *d_blob, void *hip_stream);
int32_t solo_forward_set_state(solo_forward_t *f, const int32_t *d_rooms, int32_t n, const uint8_t *d_blob, void *hip_stream);
int32_t solo_forward_levels(const solo_arrival_t *d_arrivals, const uint8_t *d_level_in, int32_t n_dgrams, int32_t n_rows,
                            int32_t default_level, solo_forward_row_t *d_rowinfo, uint8_t *d_sa_q8, uint8_t *d_level, void *hip_stream);
int32_t solo_forward_route(solo_forward_t *f, const solo_arrival_t *d_arrivals, int32_t n_dgrams, const solo_forward_row_t *d_rowinfo,
                           const uint8_t *d_sel, const int32_t *d_room, int32_t n, int32_t n_rooms,
                           solo_arrival_t *d_records, int32_t max_records, solo_send_count_t *d_send_count,
                           uint8_t *d_level_fwd, int32_t *d_slot_src, solo_forward_count_t *d_count, void *hip_stream);
/* RTCP (RFC 3550 section 6.4): reception statistics per stream, kept on the device from the arrivals solo_rtp_parse wrote, the sender's
 * packet and octet counts from the datagrams solo_rtp_pack / solo_srtp_protect left, compound SR / RR + SDES packets built from both, and
 * the peers' compound packets parsed into round-trip time and loss feedback.  A solo_rtcp_t stands beside the solo_rtp_t sessions and never
 * writes them: it reads their per-stream records and SSRC tables on the device.  One row per stream, 32 integer words (little-endian
 * uint32 unless said otherwise), then the CNAME:
 *     0 base_seq   1 max_seq   2 cycles (a multiple of 65536)   3 bad_seq   4 received   5 expected_prior   6 received_prior      (A.1)
 *     7 transit    8 jitter (scaled by 16, A.8)    9 seen: bit 0 a datagram has counted, bit 1 transit is set, bit 2 an SR was parsed
 *    10 lsr (the middle 32 bits of the peer's last SR's NTP stamp)    11 lsr_arrival (the middle 32 bits of the local time it was parsed at)
 *    12 tx_packets   13 tx_octets (wrapping)   14 tx_next (1 + the highest packet number sent)   15 tx_since (datagrams since the last build)
 *    16 .. 31 reserved, zero;   then 32 bytes: the CNAME, NUL-padded (all zero: none)
 * Object and control plane -- a row-state object like solo_vad_t.  solo_rtcp_create: NULL for n_streams <= 0.  solo_rtcp_reset: every
 * row; solo_rtcp_reset_rows: a HOST list, -1 for an index outside [0, n_streams) or listed twice; a reset leaves every word AND the CNAME
 * zero.  solo_rtcp_get_state / _set_state: a DEVICE list of rows or NULL, uint8 [n][SOLO_RTCP_STATE_BYTES + SOLO_RTCP_CNAME_BYTES], as
 * the other row objects: the hand-over of a stream to another object.  solo_rtcp_set_cname: HOST arrays, h_cname [n][32] with a name of
 * 1 .. 31 bytes, NUL-padded; ordered on hip_stream, returns when the device holds the names; -1 and nothing changed for a NULL argument,
 * n <= 0, an index outside [0, n_streams) or listed twice, an empty name or one without a NUL inside its 32 bytes.  Lifecycle, state
 * and name calls come before a graph is recorded.  Calls on one object must be ordered (same stream, or events).
 * solo_rtcp_received -- behind solo_rtp_parse: r the session that parsed, d_arrivals / d_rtp_seq / n_dgrams as parse wrote them,
 *   d_arrival_time uint32 [n_dgrams] in RTP timestamp units of the caller's clock, NULL = every datagram arrived at now_rtp.  An arrival
 *   COUNTS when its stream is inside [0, n_streams); desc = -1 counts (it was a datagram on the wire), a rejected datagram (stream = -1)
 *   is not_counted.  Per stream, its counting datagrams are processed IN INCREASING DATAGRAM INDEX, each by update_seq of RFC 3550 A.1 on
 *   the raw 16-bit sequence number (MAX_DROPOUT 3000, MAX_MISORDER 100, no probation: the bind vouched for the source), with one outcome:
 *     first            seen bit 0 was clear: init_seq (base_seq = max_seq = seq, bad_seq = 65537, cycles = 0, received = expected_prior =
 *                      received_prior = 0), accepted
 *     in_order         udelta = (seq - max_seq) mod 2^16 < 3000: cycles += 65536 if seq < max_seq; max_seq = seq; accepted
 *     dropout_pending  3000 <= udelta <= 65536 - 100 and seq != bad_seq: bad_seq = (seq + 1) mod 2^16; NOT accepted
 *     resynced         ... and seq == bad_seq: init_seq, accepted
 *     misordered       udelta > 65536 - 100 (reordered, or a duplicate of an older packet): accepted
 *   An accepted datagram adds 1 to received and then updates the jitter (A.8): transit = arrival_time - (ts_offset + seq x packet_samples)
 *   mod 2^32, from the ARRIVAL's packet number and the session's ts_offset (no wire byte is read again); if seen bit 1 is set,
 *   d = |(int32)(transit - the row's transit)| and jitter += d - ((jitter + 8) >> 4); then the row's transit = transit, bit 1 set.
 *   d_count: counted = first + in_order + misordered + dropout_pending + resynced, and not_counted.  The result equals this sequential
 *   rule for any interleaving of streams and depends on nothing but the index order.  How: a histogram per stream and the workgroup scan
 *   the bridge stages share, a scatter of the datagram indices into per-stream segments, then one wavefront per stream that puts its
 *   segment (at most SOLO_RTCP_WALK_MAX datagrams) back into index order and walks it; a stream with more gets a workgroup of its own
 *   that reads the arrival list tile by tile in index order: no lane loops over the call per datagram, the work is linear in n_dgrams
 *   plus, per flooding stream (at most n_dgrams / (SOLO_RTCP_WALK_MAX + 1) of them), one pass over the arrivals.
 *   -1 with nothing enqueued: NULL c, r or d_count; r has another stream count; n_dgrams < 0, or n_dgrams > 0 with NULL d_arrivals or
 *   d_rtp_seq; d_arrivals, d_arrival_time or d_count not 4-byte, d_rtp_seq not 2-byte aligned.  Eight short kernels on hip_stream; the
 *   scratch (8 bytes per datagram) grows, with a stream synchronisation, only when a call has more datagrams than every one before it;
 *   no host synchronisation otherwise: capturable with n_dgrams frozen (tests/test_gpu_rtcp.py: test_capture_received_tick).
 * solo_rtcp_sent -- behind solo_rtp_pack or solo_srtp_protect: r the sending session, d_records / d_send_count / max_records / d_dgrams
 *   as those calls left them.  The records of the call are min(d_send_count->records, max_records), read on the device; a negative
 *   count: d_count->sent = -1, nothing touched.  Every record k with d_dgrams[k].len > 0 and a stream inside [0, n_streams) is `sent`:
 *   tx_packets += 1, tx_octets += the RECORD's len (payload octets: no header, no tag), tx_since += 1, tx_next = max(tx_next, seq + 1);
 *   every other record is `skipped`.  Atomics, a lane per record: independent of the order.  -1: a NULL pointer, r with another stream
 *   count, max_records <= 0, a pointer not 4-byte aligned.  Two kernels, no allocation: capturable with max_records frozen
 *   (tests/test_gpu_rtcp.py: test_capture_sent_tick).
 * solo_rtcp_build -- one compound packet per listed stream, d_dgrams[i] = that of d_streams[i], back to back in d_wire, every length a
 *   multiple of 4.  d_streams: a DEVICE list under the rule of every device list (strictly increasing inside [0, n_streams), which also
 *   means none twice); a list that breaks it refuses the whole call on the device: d_count->built = -1, nothing else is touched.
 *   now: *d_now_ntp if that is given, else now_ntp (64 bits, 32.32 fixed point; A REPLAY OF A CAPTURED CALL REPEATS THE SCALAR, so a
 *   caller who captures brings the time in the device word); mid32(x) = (x >> 16) mod 2^32.
 *   refused, d_dgrams[i] = {0, 0}: the stream is not bound in r_tx, or has no CNAME (RFC 3550 makes it mandatory in every compound packet).
 *   First packet: SR (PT 200, 28 bytes) if tx_since > 0, else RR (PT 201, 8 bytes); sender SSRC = the stream's in r_tx.  SR: NTP = now,
 *   RTP timestamp = ts_offset + tx_next x packet_samples of r_tx -- the sampling instant of the packet the NEXT tick sends, an
 *   approximation of "the same instant as the NTP stamp" that is off by less than one tick --, then tx_packets and tx_octets.
 *   One report block (RC = 1, 24 bytes) iff r_rx is given, the stream is bound there and seen bit 0 is set, else RC = 0: SSRC_1 = the
 *   stream's in r_rx; by A.3 expected = cycles + max_seq - base_seq + 1, lost = (int32)(expected - received) clamped to [-0x800000,
 *   0x7FFFFF], expected_interval = expected - expected_prior, lost_interval = (int32)(expected_interval - (received - received_prior)),
 *   fraction = 0 if expected_interval == 0 or lost_interval <= 0, else min(255, (lost_interval << 8) / expected_interval); then
 *   cycles | max_seq, jitter >> 4, lsr, and DLSR = mid32(now) - lsr_arrival (both 0 while seen bit 2 is clear).
 *   SDES (PT 202, SC = 1): the same sender SSRC, item 1 (CNAME), its length, the text, one zero octet, zero-padded to a multiple of 4.
 *   Cap, as in solo_rtp_pack: packet i is written iff it ends inside wire_capacity; the offsets grow along the list, so what is written
 *   is a prefix and nothing is written at or beyond the cap; wire_capacity = 0 only counts; bytes_needed is 64 bits.  A written packet
 *   with a report block sets expected_prior = expected and received_prior = received; every written packet sets tx_since = 0.  A packet
 *   cut by the cap or refused changes no state.  d_count: built / built_needed (packets written / not refused), bytes / bytes_needed,
 *   refused, with_sr (written packets that begin with an SR).
 *   -1 with nothing enqueued: NULL c, r_tx, d_streams, d_dgrams, d_wire or d_count; a session with another stream count; n outside
 *   (0, n_streams]; wire_capacity < 0; d_streams, d_dgrams, d_wire not 4-byte, d_now_ntp or d_count not 8-byte aligned.  Four kernels
 *   (the list check, tile totals, a scan, the packets: a lane each), scratch sized at create: capturable with n frozen
 *   (tests/test_gpu_rtcp.py: test_capture_build_and_parse).
 * solo_rtcp_parse -- n_dgrams received compound packets inside d_wire at any byte alignment, a lane each; r_rx has the peers' SSRCs, r_tx
 *   (or NULL) ours.  Validity is RFC 3550 A.2 over the whole datagram; the verdict is the FIRST rule that fails, each with a counter:
 *     malformed   the range is outside [0, min(wire_bytes, 2^31 - 1)) or len < 4
 *     version     the first header's V is not 2
 *     first_type  the first header has P set or a PT other than 200 / 201
 *     then packet by packet from the first on, at byte `at`: length if at + 4 > len; version if V is not 2; length if the packet's
 *     4 x (length field + 1) bytes reach past len, if P is set on a packet that is not the last or with a pad count (the last octet) that
 *     is 0, no multiple of 4 or larger than the packet's body, or if the body is too short for what the header announces (SR: 24 + 24 RC,
 *     RR: 4 + 24 RC, BYE: 4 SC bytes behind the header).
 *   A rejected datagram changes nothing.  In an accepted one: an SR whose sender SSRC is bound in r_rx (the table search of
 *   solo_rtp_parse) gives that stream lsr = mid32(its NTP stamp), lsr_arrival = mid32(now), seen bit 2, counted sr; an unknown sender is
 *   counted unknown_ssrc and its SR skipped; its report blocks are still read.  Among several SRs of one stream in a call the one in the
 *   HIGHEST DATAGRAM INDEX wins (inside one datagram the last).  A report block (of an SR or RR) whose SSRC_n is bound in r_tx is that
 *   stream's feedback, counted blocks: d_feedback[stream] = {seen, fraction_lost, cum_lost (24 bits sign-extended), ext_high_seq, jitter,
 *   lsr, dlsr, rtt}, rtt = mid32(now) - lsr - dlsr in 1 / 65536 s, 0 where that is negative as int32, -1 where lsr == 0; the highest
 *   datagram index wins, inside a datagram the last such block; seen = the blocks the stream got in the call, | 1 << 30 if a BYE (PT 203)
 *   in the call lists the stream's SSRC of r_rx (counted bye per listed SSRC found).  EVERY row of d_feedback [n_streams] is written: a
 *   row without a block is {seen = 0 or 1 << 30, 0, 0, 0, 0, 0, 0, rtt = -1}.  SDES, APP and every other packet type are skipped by
 *   length and counted skipped.  The result does not depend on the order of the datagrams except through the index rule.
 *   -1 with nothing enqueued: NULL c, r_rx, d_feedback or d_count; a session with another stream count; n_dgrams < 0 or wire_bytes < 0;
 *   n_dgrams > 0 with NULL d_dgrams or d_wire; d_dgrams, d_feedback not 4-byte, d_now_ntp or d_count not 8-byte aligned.  Three kernels;
 *   the scratch (4 bytes per datagram) grows like that of solo_rtcp_received: capturable with n_dgrams frozen
 *   (tests/test_gpu_rtcp.py: test_capture_build_and_parse).
 * Not built: report timing and the choice of whom to report, XR, NACK / PLI / REMB, reduced-size RTCP,
 * more than one report block per packet, source probation, RTCP state in a migration blob.  INTEGRATION.md section 2 has both ticks. */
#define SOLO_RTCP_STATE_BYTES 128    /* a row's 32 words */
#define SOLO_RTCP_CNAME_BYTES 32     /* ... and its CNAME behind them in a state blob */
#define SOLO_RTCP_WALK_MAX 128       /* datagrams of one stream in one solo_rtcp_received call that a wavefront walks from its segment */
#define SOLO_RTCP_BYE (1 << 30)      /* solo_rtcp_feedback_t.seen: a BYE named the stream */
typedef struct solo_rtcp_obj solo_rtcp_t;
typedef struct { int32_t counted, first, in_order, misordered, dropout_pending, resynced, not_counted, reserved; } solo_rtcp_received_count_t;  /* 32 bytes */
typedef struct { int32_t sent, skipped, reserved[6]; } solo_rtcp_sent_count_t;                     /* 32 bytes; sent = -1: the records were refused */
typedef struct { int32_t built, built_needed; int64_t bytes, bytes_needed; int32_t refused, with_sr; } solo_rtcp_build_count_t;   /* 32 bytes; built = -1: list refused */
typedef struct { int32_t accepted, malformed, version, first_type, length, sr, blocks, unknown_ssrc, bye, skipped, reserved[6]; } solo_rtcp_parse_count_t;  /* 64 bytes */
typedef struct { int32_t seen, fraction_lost, cum_lost; uint32_t ext_high_seq, jitter, lsr, dlsr; int32_t rtt; } solo_rtcp_feedback_t;    /* 32 bytes */
/* The object's lifecycle and control plane, then its four device calls. */
solo_rtcp_t *solo_rtcp_create(int32_t n_streams);
void    solo_rtcp_destroy(solo_rtcp_t *c);
int32_t solo_rtcp_reset(solo_rtcp_t *c, void *hip_stream);
int32_t solo_rtcp_reset_rows(solo_rtcp_t *c, const int32_t *h_rows, int32_t n, void *hip_stream);
int32_t solo_rtcp_get_state(solo_rtcp_t *c, const int32_t *d_rows, int32_t n, uint8_t *d_blob, void *hip_stream);
int32_t solo_rtcp_set_state(solo_rtcp_t *c, const int32_t *d_rows, int32_t n, const uint8_t *d_blob, void *hip_stream);
int32_t solo_rtcp_set_cname(solo_rtcp_t *c, const int32_t *h_streams, int32_t n, const char *h_cname, void *hip_stream);
int32_t solo_rtcp_received(solo_rtcp_t *c, const solo_rtp_t *r, const solo_arrival_t *d_arrivals, const uint16_t *d_rtp_seq, int32_t n_dgrams,
                           const uint32_t *d_arrival_time, uint32_t now_rtp, solo_rtcp_received_count_t *d_count, void *hip_stream);
int32_t solo_rtcp_sent(solo_rtcp_t *c, const solo_rtp_t *r, const solo_arrival_t *d_records, const solo_send_count_t *d_send_count,
                       int32_t max_records, const solo_dgram_t *d_dgrams, solo_rtcp_sent_count_t *d_count, void *hip_stream);
int32_t solo_rtcp_build(solo_rtcp_t *c, const solo_rtp_t *r_tx, const solo_rtp_t *r_rx, const int32_t *d_streams, int32_t n, uint64_t now_ntp,
                        const uint64_t *d_now_ntp, solo_dgram_t *d_dgrams, uint8_t *d_wire, int64_t wire_capacity,
                        solo_rtcp_build_count_t *d_count, void *hip_stream);
int32_t solo_rtcp_parse(solo_rtcp_t *c, const solo_rtp_t *r_rx, const solo_rtp_t *r_tx, const solo_dgram_t *d_dgrams, int32_t n_dgrams,
                        const uint8_t *d_wire, int64_t wire_bytes, uint64_t now_ntp, const uint64_t *d_now_ntp,
                        solo_rtcp_feedback_t *d_feedback, solo_rtcp_parse_count_t *d_count, void *hip_stream);
/* SRTCP (RFC 3711 section 3.4): solo_srtcp_protect stands behind solo_rtcp_build and turns the compound packets into SRTCP in place,
 * solo_srtcp_unprotect stands in front of solo_rtcp_parse and turns the peers' SRTCP datagrams back into RTCP in place, so that a secured
 * session sends no RTCP in the clear and still walks no packet on the host.  An SRTCP datagram is the compound packet with its first 8
 * bytes (first header, sender SSRC) in the clear and everything from byte 8 on under AES-128 in counter mode, then ONE big-endian word
 * E << 31 | index (index: 31 bits; E = 1: encrypted), then the tag.  No MKI.  THE TAG IS ALWAYS 10 BYTES: RFC 3711 section 5.2 and RFC 4568
 * keep HMAC_SHA1_80 for SRTCP in the _32 suite as well, so there is no tag_bytes argument and the trailer is always
 * SOLO_SRTCP_TRAILER_BYTES = 4 + 10.  IV = (k_s << 16) ^ (SSRC << 64) ^ (index << 16) with SSRC = bytes 4 .. 8 and index without E;
 * keystream block j = AES(k_e, IV + j) XORed over bytes [8, len); tag = the first 10 bytes of HMAC-SHA1(k_a, bytes [0, len) as sent ||
 * the E || index word).  Session keys: the PRF of section 4.3 with rate 0 and index 0 over one direction's 30 bytes of master key ||
 * master salt, labels 3 (cipher key), 4 (authentication key), 5 (salt).
 * solo_rtcp_set_trailer -- a host switch on the RTCP object like solo_rtp_set_trailer, 0 .. 16 or exactly 20, default 0, read when a solo_rtcp_build call
 *   is issued: with a trailer T build plans every packet that is not refused as roundup4(len + T), writes the T bytes and the pad behind
 *   the packet as zero, leaves d_dgrams[i].len = len, counts the trailer in bytes and bytes_needed, and writes a packet iff all of it,
 *   trailer included, ends inside wire_capacity.  T = 0: every byte, count and state word as without the call.  -1: NULL c, or a value
 *   outside 0 .. 16 other than 20.
 * Control plane, on the solo_rtp_t session beside solo_srtp_* (it has the SSRC table) -- HOST arrays, ordered on hip_stream, the calls
 * return when the device holds the records.  Per stream: two 256-byte key records as those of SRTP (tag = 10), a send record {uint32
 * next: the index the next protected packet gets} and a receive record {int64 index: the highest authenticated, -1 = none yet; uint64
 * pending}.  They are ONE device allocation of their own, made by the first solo_srtcp_set_keys: a session without SRTCP pays nothing,
 * and solo_srtp_* allocates nothing more than before.  The host keeps "has tx / has rx" per stream and never the keys.
 *   solo_srtcp_set_keys   h_tx_master / h_rx_master: [n][30] or NULL = that direction keeps what it had; h_tx_index: [n], 0 .. 2^31, NULL
 *                    = 0 (the RFC's first index); h_rx_index: [n], -1 .. 2^31 - 1, the highest index already authenticated, NULL = -1.
 *                    Setting a tx key sets the send index, setting an rx key sets the receive record.  -1, nothing changed: NULL r or
 *                    list; n <= 0, an index outside [0, n_streams) or listed twice; both masters NULL; an initial index outside its range
 *   solo_srtcp_clear_keys  both keys of the listed streams and their send index are zeroed on the device, the receive record goes back
 *                    to "none yet".  solo_rtp_unbind does the same for its streams, solo_rtp_destroy zeroes the allocation;
 *                    solo_srtp_clear_keys does not touch it
 *   solo_srtcp_get_index  h_tx_next[i] / h_rx_index[i] = send index / receive record of listed stream i (0 / -1 without SRTCP); either may
 *                    be NULL.  With solo_srtcp_set_keys' two index arrays this is the hand-over to another session
 * solo_srtcp_protect -- datagram i belongs to d_streams[i], the list the build call had (c: the object that built; its trailer switch
 *   must stand at 14 or more).  d_build_count->built < 0 (the list was refused on the device): d_count->ok = -1 and no datagram, index
 *   or byte is touched -- which is also what keeps two lanes from sharing a send index.  d_dgrams[i].len == 0 (refused, or cut by the
 *   cap): skipped.  Then the FIRST rule that fails, each with a counter: malformed (len < 8; len no multiple of 4; the range or its 14
 *   trailer bytes outside [0, min(wire_bytes, 2^31 - 1)); a listed stream outside [0, n_streams)), no_key (no tx SRTCP key), exhausted
 *   (the stream's next is 2^31: the key has protected 2^31 packets and must be changed, RFC 3711 section 9.2).  A datagram that fails
 *   becomes {0, 0} and does not advance the index: NOTHING OF A SESSION'S LEAVES IN THE CLEAR THROUGH THIS CALL.  Otherwise index = next:
 *   [8, len) is encrypted, 0x80000000 | index goes to [len, len + 4) and the tag to [len + 4, len + 14), d_dgrams[i].len += 14,
 *   next += 1.  -1 with nothing enqueued: a NULL pointer; n outside (0, n_streams]; wire_bytes < 0; a session with another stream count;
 *   a trailer switch of c below 14; d_streams, d_dgrams, d_wire or d_count not 4-byte, d_build_count not 8-byte aligned.  Two kernels (the
 *   clear of the count, a workgroup per 256 datagrams), no allocation, no host synchronisation: capturable with n frozen, and every
 *   replay advances the indices, as it must (tests/test_gpu_srtcp.py: test_capture_rtcp_build_and_srtcp_protect).
 * solo_srtcp_unprotect -- n_dgrams datagrams inside d_wire at any byte alignment, their ranges disjoint.  The FIRST rule that fails:
 *   malformed (the range outside [0, min(wire_bytes, 2^31 - 1)), or len < 8 + 14), unknown_ssrc (bytes 4 .. 8 are not in r_rx's table:
 *   the search of solo_rtp_parse), no_key (no rx SRTCP key), replayed, auth_failed.  AUTHENTICATE FIRST: only an accepted datagram
 *   with E = 1 is decrypted, one with E = 0 is authenticated and left as it is; d_dgrams_out[i] = {offset, len - 14}, ready for
 *   solo_rtcp_parse (d_dgrams_out may be d_dgrams).  A rejected datagram keeps every wire byte and yields {0, 0}, which parse counts as
 *   malformed.
 *   THE REPLAY RULE: A DATAGRAM IS ACCEPTED ONLY IF ITS INDEX IS STRICTLY NEWER THAN EVERYTHING AUTHENTICATED FOR ITS STREAM BEFORE THIS
 *   CALL -- replayed: index <= the stream's receive record as it stood when the call began.  This is NOT the RFC's 64-packet window:
 *   RTCP has no ring behind it that would drop a replay, and a report that arrives after a newer one of the same sender is dropped,
 *   which costs nothing because the newer report supersedes it.  The verdict kernel only reads the record and raises `pending` with a
 *   64-bit atomic max; a second short kernel, a lane per stream, folds pending into index: the result does not depend on the order
 *   inside the call.  Two copies of one datagram inside one call both pass (solo_rtcp_parse's highest-index-wins rule makes the second
 *   harmless, except that `seen` counts it); the result equals a packet-by-packet receiver under the same rule whenever each stream's
 *   datagrams stand in increasing index order in the call -- so whenever a call holds at most one datagram per stream.  A newer datagram
 *   IN FRONT of an older one of the same stream lets both pass, where that receiver would drop the older.
 *   -1 with nothing enqueued: NULL r_rx or d_count; n_dgrams < 0 or wire_bytes < 0; with n_dgrams > 0 a NULL d_dgrams, d_wire or
 *   d_dgrams_out; d_dgrams, d_dgrams_out or d_count not 4-byte aligned.  Three kernels, no allocation, no host synchronisation:
 *   capturable with n_dgrams frozen (tests/test_gpu_srtcp.py: test_capture_srtcp_unprotect_and_rtcp_parse).
 * Not built: the MKI, sending with E = 0, the 64-packet replay window, AES-256, SRTCP keys and indices
 * in a migration blob. */
#define SOLO_SRTCP_TRAILER_BYTES 14  /* the E || index word (4) and the tag (10) behind every SRTCP datagram */
typedef struct { int32_t ok, skipped, malformed, unknown_ssrc, no_key, auth_failed, replayed, exhausted; } solo_srtcp_count_t;   /* 32 bytes; ok = -1: the list was refused */
/* The trailer switch of the RTCP object, the key calls of the session, then the two SRTCP device calls. */
int32_t solo_rtcp_set_trailer(solo_rtcp_t *c, int32_t trailer_bytes);
int32_t solo_srtcp_set_keys(solo_rtp_t *r, const int32_t *h_streams, int32_t n, const uint8_t *h_tx_master, const uint8_t *h_rx_master,
                            const uint32_t *h_tx_index, const int64_t *h_rx_index, void *hip_stream);
int32_t solo_srtcp_clear_keys(solo_rtp_t *r, const int32_t *h_streams, int32_t n, void *hip_stream);
int32_t solo_srtcp_get_index(solo_rtp_t *r, const int32_t *h_streams, int32_t n, uint32_t *h_tx_next, int64_t *h_rx_index, void *hip_stream);
int32_t solo_srtcp_protect(const solo_rtcp_t *c, solo_rtp_t *r_tx, const int32_t *d_streams, int32_t n,
                           const solo_rtcp_build_count_t *d_build_count, solo_dgram_t *d_dgrams, uint8_t *d_wire, int64_t wire_bytes,
                           solo_srtcp_count_t *d_count, void *hip_stream);
int32_t solo_srtcp_unprotect(solo_rtp_t *r_rx, const solo_dgram_t *d_dgrams, int32_t n_dgrams, uint8_t *d_wire, int64_t wire_bytes,
                             solo_dgram_t *d_dgrams_out, solo_srtcp_count_t *d_count, void *hip_stream);
/* AEAD_AES_128_GCM (RFC 7714) as a second transform of the SRTP and the SRTCP stage, for peers that negotiate SRTP_AEAD_AES_128_GCM
 * (DTLS-SRTP).  It is selected per stream and direction by the key that was set: a stream and direction has ONE key, the last set call
 * wins whichever transform it names, and a session may hold streams of both transforms side by side in one call.  The four device
 * calls (solo_srtp_protect / _unprotect, solo_srtcp_protect / _unprotect) keep their signatures, their -1 rules, their verdict order
 * and their count structures; every datagram of a call is counted once.  A session that never sets a GCM key allocates and enqueues
 * exactly what it did; one that holds a GCM key in a call's direction enqueues one more kernel (a workgroup per 64 datagrams) behind
 * the older transform's, in front of the fold kernel, which takes the datagrams of GCM-keyed streams and adds to the same count.
 *   The transform: tag 16 bytes, 12-byte IV, J0 = IV || 00 00 00 01, keystream block j = AES(k, IV || be32(j + 2)), tag = AES(k, J0) ^
 *   GHASH(AES(k, 0^128), AAD, ciphertext).  Keying material per direction: SOLO_SRTP_GCM_MASTER_BYTES = master key (16) || master salt
 *   (12); session key and salt by the PRF of RFC 3711 section 4.3 (rate 0, index 0) with the salt padded on the right to 14 bytes, labels
 *   0 / 2 for SRTP and 3 / 5 for SRTCP; there is no authentication key.  The 256-byte key record keeps its layout: round keys, the 12
 *   salt bytes, H where the HMAC states were, tag = 16, and a word that names the transform (0 for the older one).
 *   SRTP: IV = (00 00 || SSRC || ROC || SEQ) ^ salt; the associated data is the RTP header, 12 + 4 CC bytes and the extension block --
 *   what AES-CM leaves in the clear, so the RFC 6464 level stays readable; the plaintext is everything behind it.  On the wire: header,
 *   ciphertext, tag; d_dgrams[k].len += 16 on protect (solo_rtp_set_trailer(16) is its room), len - 16 on unprotect.  unprotect's
 *   malformed rule uses tag = 16 for a stream under a GCM rx key (and 4, as before, where stream or key is not known); the rollover
 *   estimate, the pending index and the fold kernel are those of the older transform.  The ROC is neither sent nor associated data.
 *   SRTCP: IV = (00 00 || SSRC || 00 00 || index) ^ salt.  E = 1: associated data = bytes [0, 8) || the word 0x80000000 | index, plaintext
 *   = bytes [8, len).  On the wire: bytes [0, 8), ciphertext, tag (16), and the E || index word as the LAST four bytes -- not the HMAC
 *   layout, where the word stands in front of the tag.  E = 0 (accepted, never written): associated data = the packet || the word,
 *   nothing is encrypted; on the wire packet, tag, word.  The trailer is SOLO_SRTCP_GCM_TRAILER_BYTES = 20: solo_rtcp_set_trailer(20),
 *   and solo_srtcp_protect returns -1 with nothing enqueued while c's trailer is below 20 and the session holds any GCM SRTCP tx key.
 *   unprotect: len < 8 + 14 stays the first rule; a datagram of a stream under a GCM rx key with len < 8 + 20 is malformed; the replay
 *   rule, the exhausted rule and their counters are unchanged.  d_dgrams[i].len += 20 on protect, len - 20 on unprotect.
 *   AUTHENTICATE FIRST and NOTHING OF A SESSION'S LEAVES IN THE CLEAR hold as for the older transform: a rejected datagram keeps every byte.
 * solo_srtp_set_keys_gcm / solo_srtcp_set_keys_gcm -- the semantics and refusals of solo_srtp_set_keys / solo_srtcp_set_keys with masters
 *   of [n][28] bytes and no tag_bytes argument; a tx SRTP key is refused while the session's trailer is below 16.  solo_srtp_set_keys keeps
 *   refusing every tag_bytes but 4 and 10; solo_rtp_set_trailer never goes below the tag of a keyed sender, which may now be 16.
 *   solo_srtp_clear_keys / solo_srtcp_clear_keys, solo_rtp_unbind and the get_*index calls keep their meaning for both kinds of key.
 * Graph capture: the four device calls stay capturable under GCM keys with the same frozen arguments (tests/test_gpu_srtp_gcm.py:
 *   test_capture_srtp_gcm_protect_and_unprotect, test_capture_srtcp_gcm_protect_and_unprotect).  The extra kernel is part of the
 *   captured sequence.  A graph captured before the session's first GCM key in the call's direction does not hold it and FAILS CLOSED: a
 *   datagram of a GCM-keyed stream is no_key to such a replay -- voided by protect, rejected with every byte kept by unprotect -- until
 *   the call is captured again.
 * Not built: AEAD_AES_256_GCM, the 8-byte-tag variants, MKI, RFC 6904, GCM keys in a migration blob, constant-time
 * table access. */
#define SOLO_SRTP_GCM_MASTER_BYTES 28    /* master key (16) || master salt (12): one direction's DTLS-SRTP keying material */
#define SOLO_SRTP_GCM_TAG_BYTES 16
#define SOLO_SRTCP_GCM_TRAILER_BYTES 20  /* the tag (16), then the E || index word (4) */
/* The two key calls of the transform; the device calls are those above. */
int32_t solo_srtp_set_keys_gcm(solo_rtp_t *r, const int32_t *h_streams, int32_t n, const uint8_t *h_tx_master, const uint8_t *h_rx_master,
                               const uint32_t *h_rx_roc, void *hip_stream);
int32_t solo_srtcp_set_keys_gcm(solo_rtp_t *r, const int32_t *h_streams, int32_t n, const uint8_t *h_tx_master, const uint8_t *h_rx_master,
                                const uint32_t *h_tx_index, const int64_t *h_rx_index, void *hip_stream);
/* The sender's feedback loop (solo_rate): what the peers report about our sending sets each stream's bitrate without a per-stream value
 * reaching the host.  solo_rtcp_parse leaves solo_rtcp_feedback_t [n_streams] on the device; solo_rate_update, a controller with a state
 * record per row, turns it into a target per stream; solo_batch_update_rates applies the targets to the running encoders from device
 * memory; solo_rate_send_mask turns the controller's mode into the d_send mask of solo_send_pack.  The sender's RTCP tick is
 * solo_srtcp_unprotect -> solo_rtcp_parse -> solo_rate_update -> solo_batch_update_rates -> solo_batch_encode -> solo_rate_send_mask ->
 * solo_send_pack, captured as one graph (tests/test_gpu_rate.py: test_capture_closed_loop).
 * solo_batch_update_rates -- a running stream's rate from DEVICE memory.  d_target_bps int32 [n]; position i belongs to stream
 *   d_streams[i] under the rule of every device list (strictly increasing inside [0, N)); a list that breaks it refuses the whole call
 *   on the device: d_count->applied = -1, nothing else is touched.  d_streams == NULL: n must be N, position i is stream i.  A value
 *   <= 0 means "keep": counted kept, not one byte of that stream changes.  A positive value means exactly what the same targetRate_bps
 *   means to solo_batch_update_streams on this handle: minus 1600 (800 with joint_mode 1), clamped to [5000, 100000], then setup_rate
 *   (the two SNR targets); useDTX, useMDIndex and every other word of the state stay bit for bit; counted applied.  On a 32 kHz handle a
 *   value that leaves SILK below 14000 is not built (solo_batch_update_streams refuses the whole call for it): HERE, where the host
 *   does not know the values, that position is counted refused and its stream is left untouched.  listed = n.  One lane per position.
 *   Ordering exactly as solo_batch_update_streams: hip_stream first waits for the handle's work in flight (the analysis kernels write a
 *   stream's whole state back when they end: an update that overtook them would be undone); the new rate applies from the first packet
 *   encoded after the call on hip_stream.  No allocation, no host synchronisation: capturable with n frozen.
 *   -1 with nothing enqueued: NULL b, d_target_bps or d_count; a handle without an encoder; n outside (0, N], or d_streams NULL with
 *   n != N; a pointer not 4-byte aligned.
 * solo_rate_t -- an object of its own like solo_agc_t: n_rows state records of SOLO_RATE_STATE_BYTES, the lifecycle calls of every
 *   row-state object (reset_rows: a HOST list; get_state / set_state: a device list or NULL, the blob is the records as they are).
 *   The record: int32 flags (1 started, 2 has used a report, 4 thin), target_bps, uint32 last_ehs, int32 min_rtt (2^31 - 1: none yet),
 *   idle, over, under, uint32 reports used, targets changed (both since the reset, mod 2^32), int32 the last fraction_lost and rtt
 *   used, five words the stage never writes.  The reset record is zero but for min_rtt.
 * solo_rate_update -- d_feedback [n_rows] exactly as solo_rtcp_parse wrote it; every row advances by one step and writes
 *   d_target_bps[row] = the row's new target if it changed in this call, else 0 (the input format of solo_batch_update_rates: only
 *   changed streams are touched), and d_mode[row] = 0 (both descriptions) or 1 (one description per packet, alternating).  Integers
 *   only, products in 64 bits; tests/rate_model.py is this rule in plain Python integers and the normative text where the two differ.
 *   A row, in this order, with t = target_bps:
 *   1. not started: the live words go to the reset record, t = start_bps, started is set (counted started) and the row reports a
 *      change even where nothing below moves t, so that the encoder takes the controller's start rate.
 *   2. seen has SOLO_RTCP_BYE: the live words go back to the reset record, d_target_bps = 0, d_mode = 0, counted bye; nothing below.
 *   3. the report is USED iff (seen & 0xFFFF) > 0 and (the row has used no report yet or (int32)(ext_high_seq - last_ehs) > 0): a
 *      wrap-safe test.  A row with blocks whose ext_high_seq does not advance got the same interval again: counted repeated.
 *   4. not used: idle = min(idle + 1, 2^31 - 1); in the call in which idle reaches stale_calls (> 0): t = min(t, start_bps), thin is
 *      cleared, over = under = 0, counted stale -- once, as idle goes on counting: a sender without feedback does not keep an
 *      escalated rate.
 *   5. used (counted used): idle = 0, last_ehs = ext_high_seq, p = fraction_lost clamped to 0 .. 255; rtt > 0: min_rtt = min(min_rtt,
 *      rtt); delayed = rtt_guard > 0 and rtt > 0 and rtt - min_rtt > rtt_guard (rtt -1 and 0 say nothing).  Then, counted by branch:
 *        p > hi_q8           decreased: over = over + 1 if t <= min_bps (consecutive such reports at the floor) else 0;
 *                            t = min(t - (t p >> 9), t - quantum_bps): the factor 1 - p / 512, at least a quantum
 *        p < lo_q8, not delayed, not thin
 *                            increased: over = 0; t = t + max(quantum_bps, t inc_q8 >> 8)
 *        otherwise           held: over = 0; also counted delayed where p < lo_q8 and not thin, the delay guard being what held it
 *   6. thinning, on used reports only, with thin as it stood when the step began: while thin, under = under + 1 if p < lo_q8 else 0,
 *      and under >= thin_release clears thin, over and under (counted thin_off; increases resume with the next report); while not
 *      thin, thin_after > 0 and over >= thin_after sets thin (counted thin_on).
 *   Then, on every path but BYE: t is clamped to [min_bps, max_bps] and floored to a multiple of quantum_bps; changed = the row started
 *   or t differs from the target the step began with (counted changed); thin_rows = the rows that leave the call thin; rows = n_rows.
 *   Parameters, refused (-1) unless: 1 <= min_bps <= start_bps <= max_bps <= 1000000, quantum_bps >= 1 and divides all three,
 *   0 <= lo_q8 <= hi_q8 <= 255, 0 <= inc_q8 <= 256, rtt_guard (1 / 65536 s), stale_calls, thin_after, thin_release >= 0, reserved = 0.
 *   The binding's defaults are POLICY, NOT MEASUREMENTS: lo_q8 5, hi_q8 26 and inc_q8 13 are the 2 % and 10 % thresholds and the 5 % step
 *   of the loss-based controller of the RMCAT "Google Congestion Control" draft; quantum_bps 200, rtt_guard 0, stale_calls
 *   250, thin_after 0 (thinning is opt-in), thin_release 3.  Thinning is what a multiple-description codec can do below its floor rate:
 *   one description per packet halves the wire rate, and the receiver decodes from one description as it does under loss.
 *   -1 with nothing enqueued: a NULL pointer, refused parameters, d_feedback not 16-byte, d_target_bps or d_count not 4-byte aligned.
 *   Two kernels (the clear of the count, a lane per row), the parameters travel as kernel arguments, no allocation, no host
 *   synchronisation: capturable.
 * solo_rate_send_mask -- stateless, a lane per (i, p): position i is row d_streams[i] of d_mode [n_rows], or i where d_streams is NULL;
 *   seq = first_seq + (d_seq_base ? d_seq_base[i] : 0) + p mod 2^32, as solo_send_pack numbers packets.  d_send[i][p] = 3 in mode 0; in
 *   mode 1 it is 1 (MD1) on even seq and 2 (MD2 || HB) on odd seq; ANDed with d_send_in[i][p] where that is given, so a caller's own mask
 *   (silent rooms) survives; d_send may be d_send_in.  A list that is not strictly increasing inside [0, n_rows) writes nothing (every
 *   workgroup checks it itself: the call has no object to keep a verdict in).  -1 with nothing enqueued: NULL d_mode or d_send; n_rows,
 *   n or n_packets <= 0; n > n_rows; n * n_packets >= 2^31; d_streams or d_seq_base not 4-byte aligned.  One kernel: capturable.
 * Not built: a delay-gradient / transport-wide estimator, REMB, pacing, a change of rate inside a multi-packet
 * encode call, the decoder side, controller state in a migration blob (solo_rate_get_state / _set_state is the hand-over). */
/* The records, the handle's call, the object's lifecycle, then its two device calls. */
#define SOLO_RATE_STATE_BYTES 64
typedef struct solo_rate_obj solo_rate_t;
typedef struct { int32_t applied, kept, refused, listed; } solo_rate_apply_count_t;   /* 16 bytes; applied = -1: list refused on the device */
typedef struct { int32_t min_bps, max_bps, start_bps, quantum_bps, lo_q8, hi_q8, inc_q8, rtt_guard,
                 stale_calls, thin_after, thin_release, reserved; } solo_rate_params_t;              /* 48 bytes, reserved = 0 */
typedef struct { int32_t rows, started, used, repeated, increased, decreased, held, delayed,
                 stale, bye, thin_on, thin_off, thin_rows, changed, reserved[2]; } solo_rate_count_t; /* 64 bytes */
int32_t solo_batch_update_rates(solo_batch_t *b, const int32_t *d_streams, int32_t n, const int32_t *d_target_bps,
                                solo_rate_apply_count_t *d_count, void *hip_stream);
solo_rate_t *solo_rate_create(int32_t n_rows);
void    solo_rate_destroy(solo_rate_t *rc);
int32_t solo_rate_reset(solo_rate_t *rc, void *hip_stream);
int32_t solo_rate_reset_rows(solo_rate_t *rc, const int32_t *h_rows, int32_t n, void *hip_stream);
int32_t solo_rate_get_state(solo_rate_t *rc, const int32_t *d_rows, int32_t n, uint8_t *d_blob, void *hip_stream);
int32_t solo_rate_set_state(solo_rate_t *rc, const int32_t *d_rows, int32_t n, const uint8_t *d_blob, void *hip_stream);
int32_t solo_rate_update(solo_rate_t *rc, const solo_rtcp_feedback_t *d_feedback, const solo_rate_params_t *params,
                         int32_t *d_target_bps, uint8_t *d_mode, solo_rate_count_t *d_count, void *hip_stream);
int32_t solo_rate_send_mask(const uint8_t *d_mode, int32_t n_rows, const int32_t *d_streams, int32_t n, int32_t n_packets,
                            const int32_t *d_seq_base, int32_t first_seq, const uint8_t *d_send_in, uint8_t *d_send, void *hip_stream);
/* Pipelining consecutive encode calls: with on = 1 solo_batch_encode returns without making `hip_stream` wait for the handle's
 * internal streams, so the next encode call starts while the tail of this one still runs (the caller passes different output
 * buffers to calls in flight).  Before consuming the outputs of an encode call on some stream, call
 * solo_batch_wait_encode(b, stream, which): which = 0 the most recent encode call, 1 the one before; the INPUT buffers of a
 * call must stay valid and unmodified until then as well (a stream-ordered allocator does not know the handle's internal
 * streams).  Default: off (every
 * call is complete on its stream when the next operation of that stream runs).  solo_batch_wait_encode can be captured, and for an encode
 * call inside a capture it must be (see "Graph capture"); solo_batch_set_async_join is a host switch, read when a call is issued. */
int32_t solo_batch_set_async_join(solo_batch_t *b, int32_t on);
int32_t solo_batch_wait_encode(solo_batch_t *b, void *hip_stream, int32_t which);
/* Geometry / introspection */
int32_t solo_batch_n_streams(const solo_batch_t *b);
int32_t solo_batch_slot_bytes(const solo_batch_t *b);
/* Name of the dominant kernel of the last encode / decode launch (for profiling tools). */
/* Names of the device kernels behind the four timed stages: 0 = quantiser, 1 = decoder proper (batch path; symbol extraction is
 * "solo_dec_extract_kernel"), 2 = encoder analysis, 3 = encoder high band + payload (the range coder is "solo_enc_rc_kernel"). */
const char *solo_kernel_name(int32_t which);
/* Benchmark aid: bracket every kernel of this handle with HIP events on its launch stream, and read the durations of
 * the most recent encode / decode call: ms4 = {analysis, quantiser, coding, decode} (-1 = not run yet).  solo_batch_encode
 * runs its four kernels (three timed stages: the range coder is timed with the coding stage) as a pipeline over chunks of the call's packets (several launches per kernel, overlapping in
 * time on internal streams): the encoder entries are the SUM over the launches of that kernel, and
 * solo_batch_last_encode_chunks() is the number of launches per kernel of that call. */
int32_t solo_batch_set_timing(solo_batch_t *b, int32_t on);
int32_t solo_batch_last_kernel_ms(solo_batch_t *b, float *ms4);
int32_t solo_batch_last_encode_chunks(const solo_batch_t *b);
/* Conformance probes (tests only; DEVICE pointers, default stream, synchronous).  solo_debug_l0: the fixed-point vocabulary of
 * solo_amd/csrc/solo_fix.h (the reference's SKP_SMULWB .. SKP_INVERSE32_varQ, SKP_Silk_macros.h:33-122 / SKP_Silk_Inlines.h:71-220)
 * as compiled for gfx950, out[i] = op(a[i], b[i], c[i]) with the op numbers of solo_amd/csrc/solo_l0_probe.h.
 * solo_debug_sum_sqr_shift: SKP_Silk_sum_sqr_shift (SKP_Silk_sum_sqr_shift.c:40) in its wave-cooperative form, one result pair
 * per row of `len` <= 1024 int16 samples (`stride` samples between rows). */
int32_t solo_debug_l0(int32_t op, int32_t n, const int32_t *d_a, const int32_t *d_b, const int32_t *d_c, int32_t *d_out);
int32_t solo_debug_sum_sqr_shift(const int16_t *d_x, int32_t rows, int32_t len, int32_t stride, int32_t odd_start,
                                 int32_t *d_energy, int32_t *d_shift);
/* solo_debug_waveops: the wave-level vocabulary of solo_amd/csrc/solo_wave.h in its 64-lane form (wv_sum, wv_max, wv_min, wv_row_sum,
 * wv_col_sum, wv_sum64, wv_scan_incl, wv_argmin, wv_argmax, wv_bcast, SX_UNI, SX_RDLANE / SX_WRLANE, sx_lcg_first / sx_lcg_next) as the
 * codec kernels get it.  d_v, d_aux: n_vec vectors of 64 words each (aux: the index operand of the arg functions, the high word of
 * wv_sum64, the source lane of wv_bcast; its word 0 the LCG seed, the rotation and the trip count); one wavefront per vector,
 * waves_per_block = 1 or 4 wavefronts per workgroup.  mode 0: every primitive on the raw input; mode 1: the primitives chained on each
 * other's results, straight and in a loop of (aux[0] & 7) + 1 rounds; mode 2 (waves_per_block = 4 only): the workgroup vocabulary
 * (wg_sum, wg_scan_incl, wg_total), the four vectors of a workgroup being its 256 lanes and vectors beyond n_vec zeros.  d_out: int32
 * [n_vec][rows][64], every lane's own copy of
 * every result; returns rows (27 / 18 / 3; also for n_vec == 0, which launches nothing) or a negative error.  The rows are listed in
 * tests/wave_model.py, which defines what each must hold (tests/test_gpu_wave_ops.py). */
int32_t solo_debug_waveops(int32_t mode, int32_t n_vec, int32_t waves_per_block, const int32_t *d_v, const int32_t *d_aux,
                           int32_t *d_out);
/* solo_debug_rowops: the lane exchanges of the quantiser kernel (solo_amd/csrc/solo_enc_nsq_row.h: bank-masked DPP row shifts, row
 * rotations, quad permutes) applied to 64 input words, 14 rows of 64 results (tests/test_gpu_nsq_row.py).
 * solo_debug_clock: the effective shader clock in MHz while every SIMD runs vector instructions (~1 ms): lets benchmark lines from
 * different boxes of a pool be compared (bench.py records it). */
int32_t solo_debug_rowops(const int32_t *d_in, const int32_t *d_idx, int32_t *d_out, void *hip_stream);
/* solo_debug_nsq: the quantiser kernel ALONE on freshly initialised streams -- h_in: the arguments of the reference's
 * SKP_Silk_NSQ_del_dec calls (SKP_Silk_NSQ_del_dec.c:925) as hand-over records [n_streams][n_packets][2] of 660 bytes (16 kHz API rate),
 * h_out: the kernel's output records {int32 Seed; int32 r[160]; int8 q[2][164]}; HOST pointers; returns the output record size. */
int32_t solo_debug_nsq(int32_t n_streams, int32_t n_packets, const void *h_in, void *h_out);
/* Stage probes of the encoder (tests/test_enc_stages.py): ONE stage of the launch-per-chunk pipeline alone, through the launch table of the
 * rate's build (samplerate 16000 / 32000), on streams freshly initialised with (silk_rate_bps, useMDIndex, joint, dtx, frames_per_packet); HOST
 * pointers, default stream, synchronous.  `chunk` > 0 walks the n_packets in launches of `chunk` packets, 0 is one launch.
 * solo_debug_nsq_ex: solo_debug_nsq with the rate and the init arguments (solo_debug_nsq = 16000, 12000, 0, 0, 0, 2).
 * solo_debug_analysis: h_pcm int16 [n_streams][n_packets][packet samples] -> h_nsq_in SxNsqIn[n_streams][n_packets][2], h_code_in
 *   SxCodeIn[n_streams][n_packets] (solo_amd/csrc/solo_enc_state.h, solo_enc.h); returns the SxNsqIn record size.  h_sizes (may be NULL):
 *   {SxNsqIn, SxNsqOut, SxCodeIn bytes, samples of a 40 ms packet, streams per front workgroup}; n_streams == 0 launches
 *   nothing and only fills it.
 * solo_debug_coding: h_code_in SxCodeIn[n_streams][n_packets], h_nsq_out SxNsqOut[n_streams][n_packets][2] -> h_bits
 *   [n_streams][n_packets][slot_bytes], h_nbytes int16 [n_streams][n_packets][2], h_status int32 [n_streams]; returns the SxCodeIn record size. */
int32_t solo_debug_nsq_ex(int32_t samplerate, int32_t silk_rate_bps, int32_t useMDIndex, int32_t joint, int32_t dtx, int32_t frames_per_packet,
                          int32_t n_streams, int32_t n_packets, const void *h_in, void *h_out);
int32_t solo_debug_analysis(int32_t samplerate, int32_t silk_rate_bps, int32_t useMDIndex, int32_t joint, int32_t dtx, int32_t frames_per_packet,
                            int32_t n_streams, int32_t n_packets, int32_t chunk, const int16_t *h_pcm, void *h_nsq_in, void *h_code_in,
                            int32_t *h_sizes);
int32_t solo_debug_coding(int32_t samplerate, int32_t silk_rate_bps, int32_t useMDIndex, int32_t joint, int32_t dtx, int32_t frames_per_packet,
                          int32_t n_streams, int32_t n_packets, int32_t chunk, int32_t slot_bytes, const void *h_code_in, const void *h_nsq_out,
                          uint8_t *h_bits, int16_t *h_nbytes, int32_t *h_status);
/* Stage probes of the decoder (tests/test_dec_stages.py): ONE of the two kernels of the batch path alone, through the launch table of the rate's
 * build (samplerate 16000 / 32000), on streams freshly initialised with (useMDIndex, joint, frames_per_packet); HOST pointers, default stream,
 * synchronous.  h_bits [n_streams][n_packets][slot_bytes], h_nbytes int16 [n_streams][n_packets][2], h_recv uint8 [n_streams][n_packets] (NULL:
 * everything arrived) as solo_batch_decode takes them; `chunk` > 0 walks the packets in launches of `chunk` packets, 0 is one launch.
 * solo_debug_dec_extract: the extraction step alone -> h_recs SxExtracted[n_streams][n_packets][2] (solo_amd/csrc/solo_dec.h; a record that is
 *   not usable says why in pad_[0]: 1 length, 2 sampling-rate symbol, 3 coder error, 4 pulses too large for the lane's storage, 5 symbols that
 *   depend on the bytes behind the description), h_counts (may be NULL) int32 [launches]: the description slots that carry bytes as the list
 *   kernel counted them (-1 without h_recv).  Returns the SxExtracted record size; n_streams == 0 launches nothing and only returns it.
 * solo_debug_dec_synth: the decoder proper alone, from h_recs (the extract probe's records or the caller's own), or with h_recs == NULL the
 *   single kernel that reads the symbols itself.  After every launch: h_pcm int16 [n_streams][n_packets][packet samples], h_status int32
 *   [launches][n_streams], h_state [launches][n_streams][state_bytes] = the head of every stream record, its SxDecState (NULL with
 *   state_bytes 0: not wanted).  Returns the SxExtracted record size. */
int32_t solo_debug_dec_extract(int32_t samplerate, int32_t useMDIndex, int32_t joint, int32_t frames_per_packet, int32_t n_streams,
                               int32_t n_packets, int32_t chunk, int32_t slot_bytes, const uint8_t *h_bits, const int16_t *h_nbytes,
                               const uint8_t *h_recv, void *h_recs, int32_t *h_counts);
int32_t solo_debug_dec_synth(int32_t samplerate, int32_t useMDIndex, int32_t joint, int32_t frames_per_packet, int32_t n_streams,
                             int32_t n_packets, int32_t chunk, int32_t slot_bytes, const uint8_t *h_bits, const int16_t *h_nbytes,
                             const uint8_t *h_recv, const void *h_recs, int16_t *h_pcm, int32_t *h_status, void *h_state, int32_t state_bytes);
int32_t solo_debug_clock(double *mhz_out);
/* solo_debug_fn: function-level probe of the encoder's LPC / NLSF stage functions (solo_amd/csrc/solo_fn_probe.h, which lists the
 * functions and the int32 record of each; tests/test_gpu_fn_probe.py): ONE call of stage function `fn` (4 * unit + site: a2nlsf,
 * nlsf2a_stable, msvq, burg, find_lpc at the product's call sites) per case, one wavefront per case, in the build of `samplerate`
 * (16000 / 32000).  d_in int32 [n_cases][in_words], d_out int32 [n_cases][out_words]: DEVICE pointers; runs on hip_stream and waits
 * for it.  Returns 0, -1 for an fn that does not exist, record sizes that are not the fn's, n_cases outside 0 .. 65536 or a missing
 * pointer, -2 when the launch failed.  It runs the function's device body as compiled for the probe's call, in a translation unit of its
 * own; the product kernels' specialised copies are reached by whole-encoder inputs only. */
int32_t solo_debug_fn(int32_t samplerate, int32_t fn, int32_t n_cases, const int32_t *d_in, int32_t in_words, int32_t *d_out,
                      int32_t out_words, void *hip_stream);
/* Library version string. */
const char *solo_version(void);

#ifdef __cplusplus
}
#endif
#endif

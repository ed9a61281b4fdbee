// solo_enc_pipe.h -- the encoder's host-side launch schedule: what a batch handle owns for it (three internal streams, the events that
// order them, the knobs, the bookkeeping of the previous call, the scratch) and the two schedules that run on it.  Host only; included by
// solo_api.hip behind its helpers and solo_enc_ops.h.  Zeroed with the handle: every stream, event and buffer is NULL until it exists.
#ifndef SOLO_ENC_PIPE_H
#define SOLO_ENC_PIPE_H
#define SOLO_MAX_CHUNKS 64
#define SOLO_ENC_RC_BATCH_DEFAULT 5
#define SOLO_HB_GATE_ITERS 500           // bound of the high band's wait for the next quantiser launch, ~1 us each
struct solo_enc_pipe {
    int ready;                       // enc_pipe_setup has run (at the handle's first encode call)
    const solo_enc_ops* ops;         // the handle's launch table, stream count, payload slot and samples per packet (fixed at create)
    int n_streams, slot, packet_samples;
    // three internal streams: analysis / front kernel: sA, quantiser: sB, third stage of the launch-per-chunk schedule: sC
    hipStream_t sA, sB, sC;
    hipEvent_t evFork, evJoinA[2], evJoinC[2], evA[SOLO_MAX_CHUNKS], evB[SOLO_MAX_CHUNKS], evC[SOLO_MAX_CHUNKS];
    int chunk_packets;               // packets per chunk of the launch-per-chunk schedule (env SOLO_ENC_CHUNK, default 1; 0 = one chunk)
    int rc_batch;                    // packets per range-coder launch of the launch-per-chunk schedule (env SOLO_ENC_RC_BATCH; 1 = one launch per chunk)
    int group_streams;               // streams per launch group (env SOLO_ENC_GROUP; default: launch per chunk 8192, persistent = what is resident at once)
    int gate;                        // env SOLO_ENC_GATE: the front / next analysis launch starts once the quantiser's workgroups are resident
    int async_join;                  // solo_batch_set_async_join: encode returns without joining its streams into the caller's
    unsigned int enc_seq;            // encode calls so far (selects the join-event set)
    unsigned long long join_cap[2];  // the graph capture each join-event set (and with it evC[]) was last recorded in, 0 = on running streams
    int evC_valid;                   // chunks of the previous call whose coding-done events are recorded
    int last_np, last_cp;            // packets / packets per chunk of the previous call (layout of the hand-over records)
    hipEvent_t tev[3][SOLO_MAX_CHUNKS][2];   // timing brackets per kernel type / launch (created with set_timing)
    int tev_ready, ev_enc, last_chunks;      // ... exist / bracket a call / launches per kernel of the previous call
    unsigned int* d_started;         // per launch slot: workgroups of the quantiser launches that have started (running count)
    unsigned int started_target[SOLO_MAX_CHUNKS];
    void* d_nsq_ring;                // emission-ring scratch of the quantiser launches (one launch group of streams; frame-local data)
    void* d_rc_scratch;              // range-coder byte buffers of one coding launch (the launches of a call run in order on sC)
    void* d_enc_work;                // hand-over records of one call: SxNsqIn[N][P][2] | SxNsqOut[N][P][2] | SxCodeIn[N][P]
    size_t rc_scratch_bytes, enc_work_bytes;
    // persistent schedule (calls of two or more packets; off unless env SOLO_ENC_PERSIST=1 turns it on): per-stream hand-over flags, tickets
    int persist;
    int persist_group;               // streams per launch group: all of a group's front workgroups are resident beside its quantiser's
    unsigned int* d_flags;           // ana[n_streams] | nsq[n_streams / 4 + 1] | prog[n_streams] | err[4]
    unsigned int ticket;             // packets encoded by persistent calls so far (mod 2^32): the flag words are never reset
    unsigned int final_wait_ticks;   // env SOLO_ENC_FINAL_WAIT_US: bound of the front kernel's wait for the quantiser's last packets (100 MHz ticks)
    int front_defer;                 // SOLO_ENC_FINAL_WAIT_US=-1
    void* d_nsq_stage;               // the persistent quantiser's staging records (one launch group)
    void* d_front_scratch;           // byte buffers of the front kernel's in-wave range coder (one launch group)
};
#define ENC_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)
static hipError_t enc_events_create(hipEvent_t* ev, int n, unsigned int flags) {      // (those that do not exist yet)
    for (int i = 0; i < n; i++) if (!ev[i]) ENC_TRY(hipEventCreateWithFlags(&ev[i], flags));
    return hipSuccess;
}
static void enc_events_destroy(hipEvent_t* ev, int n) {
    for (int i = 0; i < n; i++) if (ev[i]) (void)hipEventDestroy(ev[i]);
}
// Releases whatever the pipe holds -- complete, partly built or nothing -- and leaves it as a new handle has it (the async-join setting stays)
static void enc_pipe_destroy(solo_enc_pipe* p) {
    hipStream_t* const streams[3] = {&p->sA, &p->sB, &p->sC};
    for (hipStream_t* s : streams) if (*s) (void)hipStreamSynchronize(*s);
    for (hipStream_t* s : streams) if (*s) (void)hipStreamDestroy(*s);
    enc_events_destroy(&p->evFork, 1); enc_events_destroy(p->evJoinA, 2); enc_events_destroy(p->evJoinC, 2);
    enc_events_destroy(p->evA, SOLO_MAX_CHUNKS); enc_events_destroy(p->evB, SOLO_MAX_CHUNKS); enc_events_destroy(p->evC, SOLO_MAX_CHUNKS);
    enc_events_destroy(&p->tev[0][0][0], 3 * SOLO_MAX_CHUNKS * 2);
    dev_free(p->d_started); dev_free(p->d_nsq_ring); dev_free(p->d_rc_scratch); dev_free(p->d_enc_work);
    dev_free(p->d_flags); dev_free(p->d_front_scratch); dev_free(p->d_nsq_stage);
    const int async_join = p->async_join;
    memset(p, 0, sizeof(*p));
    p->async_join = async_join;
}
static hipError_t enc_pipe_create(solo_enc_pipe* p) {
    const solo_enc_ops* ops = p->ops;
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);            // hi = numerically lowest = greatest priority
    ENC_TRY(hipStreamCreateWithPriority(&p->sA, hipStreamNonBlocking, lo));
    ENC_TRY(hipStreamCreateWithPriority(&p->sB, hipStreamNonBlocking, hi));
    ENC_TRY(hipStreamCreateWithPriority(&p->sC, hipStreamNonBlocking, lo));
    const unsigned int nt = hipEventDisableTiming;
    ENC_TRY(enc_events_create(&p->evFork, 1, nt)); ENC_TRY(enc_events_create(p->evJoinA, 2, nt)); ENC_TRY(enc_events_create(p->evJoinC, 2, nt));
    ENC_TRY(enc_events_create(p->evA, SOLO_MAX_CHUNKS, nt)); ENC_TRY(enc_events_create(p->evB, SOLO_MAX_CHUNKS, nt)); ENC_TRY(enc_events_create(p->evC, SOLO_MAX_CHUNKS, nt));
    int dev = 0, ncu = 0;
    ENC_TRY(hipGetDevice(&dev));
    ENC_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    // SOLO_ENC_PERSIST=1: the persistent schedule (two kernels per call that hand packets over through flags) instead of one launch per
    // chunk and stage.  Bit-exact and deadlock-free by construction, but measured SLOWER (54 - 60 against 50.5 ms per 4096 x 50 packets:
    // DESIGN.md section 9 has the trace): it removes the launch tails, but it also fixes the SIMD's population at five dependent
    // chains, where the launch-per-chunk schedule reaches nine.  Off unless asked for.
    p->persist = env_int("SOLO_ENC_PERSIST", 0) != 0;
    p->chunk_packets = env_int("SOLO_ENC_CHUNK", 1);
    if (p->chunk_packets < 0) p->chunk_packets = 1;
    // SOLO_ENC_RC_BATCH: packets per range-coder launch.  The coder is latency bound: one launch over k chunks takes about as long as
    // one chunk's.  What its launch per chunk did for the schedule -- hold the next high band back until the quantiser launch that
    // starts at the same moment is resident -- a bounded gate in front of the high band does directly (- 5 %).
    // 1 = a coder launch behind every chunk's high band, no gate.
    p->rc_batch = env_int("SOLO_ENC_RC_BATCH", SOLO_ENC_RC_BATCH_DEFAULT);
    if (p->rc_batch < 1) p->rc_batch = 1;
    if (p->rc_batch > ops->rc_batch_max) p->rc_batch = ops->rc_batch_max;
    // launch per chunk: the residency gate (hold analysis chunk c + 1 until the quantiser launch of chunk c is resident) costs 3 % with 256
    // quantiser workgroups per chunk: off unless asked for.  Persistent: ONE gate per launch group, in front of the front kernel -- the
    // quantiser's wavefronts have to be resident before 4096 front workgroups take every register of the device: on unless turned off.
    p->gate = getenv("SOLO_ENC_GATE") ? (env_int("SOLO_ENC_GATE", 0) != 0) : -1;      // (-1: the schedule's default)
    // streams per launch group.  Launch per chunk: 8192 (one group of 8192 takes 120 ms per 50 packets, two of 4096 take 134).  Persistent:
    // what is resident at once -- front workgroups per compute unit (LDS-bound: 16 at the 16 kHz rate, 9 at 32 kHz) x compute units, a
    // multiple of the quantiser's four streams per wavefront: a larger group's last workgroups would only start when the first ones have
    // finished ALL their packets, while their quantiser wavefronts held registers from the start
    const int g_env = env_int("SOLO_ENC_GROUP", -1);
    p->group_streams = g_env >= 0 ? g_env : 8192;
    p->persist_group = g_env > 0 ? ((g_env + 3) & ~3) : ((ops->front_per_cu * (ncu > 0 ? ncu : 256)) & ~3);
    if (p->persist_group < 4) p->persist_group = 4;
    {
        // (-1, tests: the front launch codes nothing -- no look at the quantiser's flags at all --, the second launch every packet)
        const long us = env_int("SOLO_ENC_FINAL_WAIT_US", 20000);
        p->front_defer = us < 0;
        p->final_wait_ticks = (unsigned int)((us < 0 ? 0 : (us > 10000000 ? 10000000 : us)) * 100);
    }
    {   // the quantiser launches of a call run one after the other on sB: one ring, sized for the largest launch group
        int gs = (p->group_streams > 0 && p->group_streams < p->n_streams) ? p->group_streams : p->n_streams;
        if (p->persist && p->persist_group > gs) gs = p->persist_group < p->n_streams ? p->persist_group : p->n_streams;
        ENC_TRY(hipMalloc(&p->d_nsq_ring, ops->nsq_ring_bytes(gs)));
    }
    ENC_TRY(hipMalloc((void**)&p->d_started, SOLO_MAX_CHUNKS * sizeof(unsigned int)));
    ENC_TRY(hipMemset(p->d_started, 0, SOLO_MAX_CHUNKS * sizeof(unsigned int)));
    if (p->persist) {
        const size_t nflags = (size_t)p->n_streams * 2 + (size_t)p->n_streams / 4 + 1 + 4;
        ENC_TRY(hipMalloc((void**)&p->d_flags, nflags * sizeof(unsigned int)));
        ENC_TRY(hipMemset(p->d_flags, 0, nflags * sizeof(unsigned int)));
        const int gs = p->persist_group < p->n_streams ? p->persist_group : p->n_streams;
        ENC_TRY(hipMalloc(&p->d_front_scratch, ops->front_scratch_bytes(gs)));
        ENC_TRY(hipMalloc(&p->d_nsq_stage, ops->nsq_stage_bytes(gs)));
    }
    return hipSuccess;
}
// one-time set-up of a handle's encoder pipeline: internal streams, events, knobs (documented in INTEGRATION.md section 5), scratch.
// All or nothing: after a failure the pipe holds nothing (timing brackets included) and is not ready, the next encode call tries again.
static int32_t enc_pipe_setup(solo_enc_pipe* p, const solo_enc_ops* ops, int n_streams, int slot, int packet_samples) {
    p->ops = ops; p->n_streams = n_streams; p->slot = slot; p->packet_samples = packet_samples;
    const hipError_t e = enc_pipe_create(p);
    if (e != hipSuccess) enc_pipe_destroy(p);
    p->ready = e == hipSuccess;
    return -(int32_t)e;
}
// The graph capture `st` is recording into, 0 when it is not capturing.  The events that order one encode call of a handle against the
// next (evJoinA / evJoinC / evC) mean something only inside the context they were recorded in: recorded in a capture they are nodes of
// that graph and order nothing outside it, and the runtime refuses (hipErrorStreamCaptureIsolation) an internal stream that has joined a
// capture and waits for an event it recorded before.  So an encode call waits for the previous call's events only when both were issued
// in ONE context -- both on running streams, or both in the same capture.  Across the boundary the caller's stream is the order: a graph
// launch runs as a whole where it stands in its stream (include/solo_mi355x.h, "Graph capture").  (evDecDone needs none of this: a
// decode call runs on the caller's stream alone, and the runtime takes its wait for an event of a running stream into a capture.)
static unsigned long long stream_capture(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    if (hipStreamGetCaptureInfo(st, &cs, &id) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return cs == hipStreamCaptureStatusActive ? (id ? id : ~0ull) : 0;
}
// The join-event set (and verdict word) of an encode call of this pipe: which = -1 the call that is being issued, 0 the most recent
// one, 1 the one before -- two sets, used in turn, so that two calls can be in flight with asynchronous joins.  For an earlier call:
// -1 where there was none, or where it was issued in another context than `cap` (stream_capture: nothing to wait for there).
static int enc_pipe_call_set(const solo_enc_pipe* p, int which, unsigned long long cap) {
    if (which < 0) return (int)(p->enc_seq & 1u);
    if (which > 1 || p->enc_seq <= (unsigned int)which) return -1;
    const int js = (int)((p->enc_seq - 1u - (unsigned int)which) & 1u);
    return p->join_cap[js] == cap ? js : -1;
}
// Makes `s` (in context `cap`) wait for the end of an earlier encode call, which = 0 or 1 as above: for its last launch on sA
// (ENC_END_A) and / or on its last stream, sC or, persistent, sB (ENC_END_C).  Nothing where enc_pipe_call_set has nothing.
enum { ENC_END_A = 1, ENC_END_C = 2, ENC_END = 3 };
static hipError_t enc_pipe_wait(solo_enc_pipe* p, hipStream_t s, unsigned long long cap, int which, int ends) {
    const int js = enc_pipe_call_set(p, which, cap);
    if (js < 0) return hipSuccess;
    if (ends & ENC_END_A) ENC_TRY(hipStreamWaitEvent(s, p->evJoinA[js], 0));
    if (ends & ENC_END_C) ENC_TRY(hipStreamWaitEvent(s, p->evJoinC[js], 0));
    return hipSuccess;
}
// Fork: the internal streams start behind everything on the caller's, sA and sB also behind the given ends of the previous call (in
// the same context).  From here on a call does not return before enc_pipe_join: every error goes into its lerr and falls through to it.
static hipError_t enc_pipe_fork(solo_enc_pipe* p, hipStream_t st, unsigned long long cap, bool third_stream, int prev_ends_a, int prev_ends_b) {
    ENC_TRY(hipEventRecord(p->evFork, st));
    ENC_TRY(hipStreamWaitEvent(p->sA, p->evFork, 0));
    ENC_TRY(hipStreamWaitEvent(p->sB, p->evFork, 0));
    if (third_stream) ENC_TRY(hipStreamWaitEvent(p->sC, p->evFork, 0));
    ENC_TRY(enc_pipe_wait(p, p->sA, cap, 0, prev_ends_a));
    return enc_pipe_wait(p, p->sB, cap, 0, prev_ends_b);
}
// Join: the call's ends are recorded (sA, and `tail`: the stream whose last launch waits for sB's -- sC, or sB itself) under the context
// it was issued in, and the caller's stream waits for them unless joins are asynchronous.  After a refused launch or event call (lerr)
// too: whatever was enqueued so far still runs, nothing of this call is left forked -- that would invalidate a capture -- (sB as well,
// which the tail's last launch may not have waited for), and the next call finds enc_seq advanced and the chunk-wise guards dropped.
static int32_t enc_pipe_join(solo_enc_pipe* p, hipStream_t st, unsigned long long cap, hipStream_t tail, hipError_t lerr, int guarded, int chunks, bool timed) {
    const bool ok = lerr == hipSuccess;
    const int js = enc_pipe_call_set(p, -1, cap);
    p->enc_seq++;
    p->join_cap[js] = cap;
    p->evC_valid = ok ? guarded : 0;      // (guarded: the chunks whose evC[] the next call may wait for one by one)
    (void)hipEventRecord(p->evJoinA[js], p->sA);
    (void)hipEventRecord(p->evJoinC[js], tail);
    if (!p->async_join || !ok) {
        (void)hipStreamWaitEvent(st, p->evJoinA[js], 0);
        (void)hipStreamWaitEvent(st, p->evJoinC[js], 0);
    }
    if (!ok && hipEventRecord(p->evFork, p->sB) == hipSuccess) (void)hipStreamWaitEvent(st, p->evFork, 0);
    p->last_chunks = ok ? chunks : 0;
    if (timed && ok) p->ev_enc = 1;
    return -(int32_t)(ok ? hipGetLastError() : lerr);
}
// What a launch works on: `ns` streams from compact position s0 of the call, every array stream-major.  A whole call is one of these
// (s0 = 0); streams beyond the launch group are processed group after group, a group is the same launch on offset pointers.
struct enc_rows {
    int s0, ns;
    void* states;                    // the first stream's state; a subset call: the handle's first, the streams are map[0 .. ns)
    const int32_t* map; const int16_t* pcm;
    void *nin, *nout, *cin;          // hand-over records
    uint8_t* bits; int16_t* nbytes; int32_t* status;       // (status may be NULL)
};
// group g of a call's rows in groups of G streams (a subset call: groups of compact positions)
static enc_rows enc_group(const solo_enc_pipe* p, const enc_rows& call, int n_packets, int g, int G) {
    const solo_enc_ops* ops = p->ops;
    enc_rows r = call;
    r.s0 = g * G;
    r.ns = (r.s0 + G <= call.ns) ? G : call.ns - r.s0;
    const size_t pk0 = (size_t)r.s0 * (size_t)n_packets;                             // first packet record of the group
    if (call.map) r.map = call.map + r.s0;
    else r.states = (char*)call.states + (size_t)r.s0 * ops->state_bytes;
    r.pcm = call.pcm + pk0 * (size_t)p->packet_samples;
    r.nin = (char*)call.nin + pk0 * 2 * ops->nsq_in_bytes;
    r.nout = (char*)call.nout + pk0 * 2 * ops->nsq_out_bytes;
    r.cin = (char*)call.cin + pk0 * ops->code_in_bytes;
    r.bits = call.bits + pk0 * (size_t)p->slot;
    r.nbytes = call.nbytes + pk0 * 2;
    if (call.status) r.status = call.status + r.s0;
    return r;
}
// Persistent schedule of one call: per launch group ONE quantiser launch (sB) and ONE front launch (sA) that hand packets to each other
// through flags while they run (solo_enc_kernels.h), then the front kernel once more behind the quantiser (mode 1: what a bounded wait
// left undone -- nothing, normally).
static int32_t enc_pipe_run_persist(solo_enc_pipe* p, const enc_rows& call, int n_packets, bool timing, hipStream_t st) {
    const solo_enc_ops* ops = p->ops;
    // not in a graph: the tickets are host counters passed by value, a replay would find the flags of the replay before it already raised
    if (stream_capture(st) != 0) return -(int32_t)hipErrorStreamCaptureUnsupported;
    const int G = p->persist_group, ngroups = (p->n_streams + G - 1) / G;
    const bool tm = timing && p->tev_ready && ngroups <= SOLO_MAX_CHUNKS;
    unsigned int *ana = p->d_flags, *nsqf = ana + p->n_streams, *prog = nsqf + (size_t)p->n_streams / 4 + 1, *err = prog + p->n_streams;
    const unsigned int ticket0 = p->ticket;
    p->ticket += (unsigned int)n_packets;
    p->last_np = n_packets; p->last_cp = 0;
    // (the previous call, of either schedule, has read its hand-over records to the end)
    hipError_t lerr = enc_pipe_fork(p, st, 0, false, ENC_END_C, ENC_END);
    for (int g = 0; g < ngroups && lerr == hipSuccess; g++) {
        const enc_rows r = enc_group(p, call, n_packets, g, G);
        const int c = g % SOLO_MAX_CHUNKS;
        unsigned int *g_ana = ana + r.s0, *g_nsqf = nsqf + r.s0 / 4, *g_prog = prog + r.s0;
        // the front kernel first; the quantiser's launch is held until the front workgroups have started (they fill every compute unit
        // up to one 128-register hole per SIMD, which is where the quantiser's wavefronts then go: solo_nsq_row.hip, "Residency")
        // (sB comes up to where sA stands -- behind the previous group's last launch -- before it starts counting)
        if ((lerr = hipEventRecord(p->evA[c], p->sA)) != hipSuccess) break;
        if ((lerr = hipStreamWaitEvent(p->sB, p->evA[c], 0)) != hipSuccess) break;
        if (tm) (void)hipEventRecord(p->tev[0][c][0], p->sA);
        if ((lerr = ops->front(r.states, r.pcm, r.ns, n_packets, r.nin, r.cin, r.nout, g_ana, g_nsqf, g_prog, ticket0, p->front_defer ? 2 : 0, p->final_wait_ticks,
                               p->slot, r.bits, r.nbytes, r.status, p->d_front_scratch, &p->d_started[c], p->sA)) != hipSuccess) break;
        p->started_target[c] += (unsigned int)((r.ns + ops->front_waves - 1) / ops->front_waves);
        if (tm) (void)hipEventRecord(p->tev[0][c][1], p->sA);
        if (p->gate != 0) (void)solo_launch_gate(&p->d_started[c], p->started_target[c], p->sB);
        if (tm) (void)hipEventRecord(p->tev[1][c][0], p->sB);
        if ((lerr = (hipError_t)ops->nsq_persist(r.states, r.nin, r.nout, r.ns, n_packets, NULL, p->d_nsq_ring, g_ana, g_nsqf, ticket0, err, p->d_nsq_stage, p->sB)) != hipSuccess) break;
        if (tm) (void)hipEventRecord(p->tev[1][c][1], p->sB);
        if ((lerr = hipEventRecord(p->evB[c], p->sB)) != hipSuccess) break;
        if ((lerr = hipStreamWaitEvent(p->sA, p->evB[c], 0)) != hipSuccess) break;
        if (tm) (void)hipEventRecord(p->tev[2][c][0], p->sA);
        lerr = ops->front(r.states, r.pcm, r.ns, n_packets, r.nin, r.cin, r.nout, g_ana, g_nsqf, g_prog, ticket0, 1, 0u, p->slot, r.bits, r.nbytes, r.status,
                          p->d_front_scratch, NULL, p->sA);
        if (tm) (void)hipEventRecord(p->tev[2][c][1], p->sA);
    }
    return enc_pipe_join(p, st, 0, p->sB, lerr, 0, ngroups <= SOLO_MAX_CHUNKS ? ngroups : 0, tm);
}
// Launch per chunk: chunk c of the call's packets goes analysis (stream sA) -> quantiser (sB) -> high band, range coder (sC).  A_c
// follows A_{c-1}, B_c follows A_c and B_{c-1}, C_c follows B_c and C_{c-1}; so the quantiser of chunk c (one wave per SIMD, latency
// bound) runs next to the analysis of chunk c + 1 and the coding of chunk c - 1 (instruction bound): they share the SIMDs.  The
// kernels of different types touch disjoint parts of the stream records.  The caller's stream is forked / joined by events.
struct enc_chunks {                  // one call's cut into chunks, fixed before its first launch
    int np, cp, nchunks, kc, kb_cap, lag;    // packets, packets per chunk, chunks; chunks / packets per range-coder launch at the most
    // the third stage's shape.  kc == 1: ops->coding (high band and coder in one launch) behind every chunk's quantiser.  kc > 1: the
    // high band of a chunk (ops->hb), behind the batch's (the call's) last chunk the range coder of all of its packets (ops->rc_batch)
    // -- and that ONE CHUNK LATE (lag = 1), behind a gate, see enc_third_stage.  (batched without lag: builds for the section tools.)
    bool batched, tm;                // (tm: timing brackets around every launch)
    const uint32_t* verdict;         // of a subset call's list
};
struct enc_rc_batch { int pb, hb_end, idx_b; };     // the open batch of the coder: its first packet, the end of its chunks with a high-band launch, its first event slot
#ifdef SX_EXPERIMENTS     // builds for the section tools only (tools/build_stops.sh): SOLO_EXP_SKIP bit 0 = no quantiser, bit 1 = no third stage, bit 2 = no range coder -- wrong output
static int enc_exp_skip() { static const int v = env_int("SOLO_EXP_SKIP", 0); return v; }
#else
constexpr int enc_exp_skip() { return 0; }
#endif
// Third stage of chunk cc (event slot idx) on sC, behind its quantiser launch.  closes: the chunk is the last of its coder batch: evC[]
// of a batch's chunks are recorded only behind its coder launch, which reads their hand-over records.  gate_slot >= 0 (lag = 1): the
// slot of the NEXT chunk's quantiser launch, which starts when this chunk's ends; the high band is held behind a gate until that launch
// is resident: its 4096 workgroups would take the register holes the quantiser's wavefronts need.  The gate gives up after ~0.5 ms
// (sC has that much slack per chunk).
static hipError_t enc_third_stage(solo_enc_pipe* p, const enc_rows& r, const enc_chunks& k, enc_rc_batch& o, int cc, int idx, bool closes, int gate_slot) {
    const solo_enc_ops* ops = p->ops;
    const int c = idx % SOLO_MAX_CHUNKS, p0 = cc * k.cp, pc = (p0 + k.cp <= k.np) ? k.cp : k.np - p0, skip = enc_exp_skip();
    ENC_TRY(hipStreamWaitEvent(p->sC, p->evB[c], 0));
    if (gate_slot >= 0) (void)solo_launch_gate_for(&p->d_started[gate_slot], p->started_target[gate_slot], SOLO_HB_GATE_ITERS, p->sC);
    if (k.tm) (void)hipEventRecord(p->tev[2][c][0], p->sC);
    if (!k.batched) {
        if (!(skip & 2)) ENC_TRY(ops->coding(r.states, r.cin, r.nout, r.ns, k.np, p0, pc, p->slot, r.bits, r.nbytes, r.status, p->d_rc_scratch, r.map, k.verdict, p->sC));
    } else {
        if (!(skip & 2)) ENC_TRY(ops->hb(r.states, r.cin, r.nout, r.ns, k.np, p0, pc, o.pb, k.kb_cap, k.cp, p->d_rc_scratch, r.map, k.verdict, p->sC));
        o.hb_end = p0 + pc;
        if (closes && !(skip & 6)) ENC_TRY(ops->rc_batch(r.states, r.cin, r.nout, r.ns, k.np, o.pb, o.hb_end - o.pb, k.kb_cap, k.cp, p->slot, r.bits, r.nbytes, r.status, p->d_rc_scratch, r.map, k.verdict, p->sC));
    }
    if (k.tm) (void)hipEventRecord(p->tev[2][c][1], p->sC);
    for (int i = o.idx_b; closes && i <= idx; i++) ENC_TRY(hipEventRecord(p->evC[i % SOLO_MAX_CHUNKS], p->sC));
    if (closes) { o.pb = o.hb_end; o.idx_b = idx + 1; }
    return hipSuccess;
}
// One launch group's chunks, event slots idx0 ...  guarded: chunks of the PREVIOUS call whose coding of the same hand-over records
// this call's analysis waits for one by one (evC[]).  A refused launch or event call ends the loop; the chunks whose quantiser is
// enqueued still get their third stage, the chunks whose high band is enqueued are still coded.
static hipError_t enc_group_chunks(solo_enc_pipe* p, const enc_rows& r, const enc_chunks& k, int idx0, int guarded) {
    const solo_enc_ops* ops = p->ops;
    enc_rc_batch o = {0, 0, idx0};
    int nb = 0, nc = 0, skip = enc_exp_skip();      // nb, nc: chunks whose quantiser / third stage is enqueued
    auto closes = [&](int cc) { return (cc + 1) % k.kc == 0 || cc + 1 == k.nchunks; };
    hipError_t lerr = hipSuccess;
    for (int cc = 0; cc < k.nchunks && lerr == hipSuccess; cc++) {
        const int idx = idx0 + cc, c = idx % SOLO_MAX_CHUNKS, cprev = (idx + SOLO_MAX_CHUNKS - 1) % SOLO_MAX_CHUNKS;     // event / counter slot
        const int p0 = cc * k.cp, pc = (p0 + k.cp <= k.np) ? k.cp : k.np - p0;
        if (cc < guarded && (lerr = hipStreamWaitEvent(p->sA, p->evC[c], 0)) != hipSuccess) break;      // (previous call: its coding of this chunk's records is done)
        if (idx > 0 && p->gate > 0) (void)solo_launch_gate(&p->d_started[cprev], p->started_target[cprev], p->sA);
        if (k.tm) (void)hipEventRecord(p->tev[0][c][0], p->sA);
        if ((lerr = ops->analysis(r.states, r.pcm, r.ns, k.np, p0, pc, r.nin, r.cin, r.map, k.verdict, p->sA)) != hipSuccess) break;
        if (k.tm) (void)hipEventRecord(p->tev[0][c][1], p->sA);
        if ((lerr = hipEventRecord(p->evA[c], p->sA)) != hipSuccess) break;
        if ((lerr = hipStreamWaitEvent(p->sB, p->evA[c], 0)) != hipSuccess) break;
        if (k.tm) (void)hipEventRecord(p->tev[1][c][0], p->sB);
        if (!(skip & 1)) {
            if ((lerr = (hipError_t)ops->nsq(r.states, r.nin, r.nout, r.ns, k.np, p0, pc, &p->d_started[c], p->d_nsq_ring, r.map, k.verdict, p->sB)) != hipSuccess) break;
            p->started_target[c] += (unsigned int)ops->nsq_workgroups(r.ns);     // workgroups of this launch, counted once it is enqueued
        }
        if (k.tm) (void)hipEventRecord(p->tev[1][c][1], p->sB);
        if ((lerr = hipEventRecord(p->evB[c], p->sB)) != hipSuccess) break;
        nb = cc + 1;
        // third stage on sC: this chunk's, or (lag = 1) the one before's behind a gate on this chunk's quantiser launch
        if (cc >= k.lag) { nc = cc - k.lag + 1; lerr = enc_third_stage(p, r, k, o, cc - k.lag, idx - k.lag, closes(cc - k.lag), k.lag ? c : -1); }
    }
    for (; nc < nb; nc++) {          // the lagging chunk (no quantiser launch follows it: no gate)
        const hipError_t e = enc_third_stage(p, r, k, o, nc, idx0 + nc, closes(nc), -1);
        if (lerr == hipSuccess) lerr = e;
    }
    if (lerr != hipSuccess && k.kc > 1 && o.hb_end > o.pb)       // a refused launch: the chunks whose high band is enqueued are still coded
        (void)ops->rc_batch(r.states, r.cin, r.nout, r.ns, k.np, o.pb, o.hb_end - o.pb, k.kb_cap, k.cp, p->slot, r.bits, r.nbytes, r.status, p->d_rc_scratch, r.map, k.verdict, p->sC);
    return lerr;
}
// The launch-per-chunk schedule of one call (call.map: of a subset call, its list already checked on `st` into *verdict).
static int32_t enc_pipe_run_chunks(solo_enc_pipe* p, const enc_rows& call, int n_packets, const uint32_t* verdict, bool timing, hipStream_t st) {
    enc_chunks k;
    k.np = n_packets; k.verdict = verdict;
    k.cp = p->chunk_packets > 0 ? p->chunk_packets : n_packets;
    k.nchunks = (n_packets + k.cp - 1) / k.cp;
    if (k.nchunks > SOLO_MAX_CHUNKS) { k.cp = (n_packets + SOLO_MAX_CHUNKS - 1) / SOLO_MAX_CHUNKS; k.nchunks = (n_packets + k.cp - 1) / k.cp; }
    // the previous call's events are waited for only inside one context (stream_capture); on the other side of a capture this call
    // starts behind everything of it through the fork from `st`
    const unsigned long long cap = stream_capture(st);
    // chunks per range-coder launch: whole chunks, SOLO_ENC_RC_BATCH packets at the most; 1 (a call of one chunk, and a call that is
    // captured into a graph: the gate's target is a running count passed by value): ops->coding per chunk
    k.kc = k.nchunks > 1 && !cap && p->rc_batch / k.cp > 1 ? (p->rc_batch / k.cp < k.nchunks ? p->rc_batch / k.cp : k.nchunks) : 1;
    k.kb_cap = k.kc * k.cp;
    k.batched = k.kc > 1 || (enc_exp_skip() & 4);
    k.lag = k.kc > 1 && !(enc_exp_skip() & 1);
    const int G = p->group_streams > 0 ? p->group_streams : call.ns, ngroups = (call.ns + G - 1) / G;
    k.tm = timing && p->tev_ready && (size_t)ngroups * (size_t)k.nchunks <= SOLO_MAX_CHUNKS;     // (per-launch timing brackets: one per event slot)
    {   // scratch of one coding launch: the byte buffers of its descriptions (sC: a coding launch of the previous call may still read the old one)
        const int gs = (p->group_streams > 0 && p->group_streams < p->n_streams) ? p->group_streams : p->n_streams;
        const hipError_t e = grow_scratch(p->d_rc_scratch, p->rc_scratch_bytes, p->ops->rc_scratch_bytes(gs, k.kb_cap), p->sC);
        if (e != hipSuccess) return -(int32_t)e;
    }
    // The hand-over records of chunk c may be written once the PREVIOUS call's coding of its chunk c has read them (evC[c]) -- where
    // that call laid them out as this one does: a single-group call of every stream with the same packets and chunks, issued in the
    // same context.  Otherwise (another layout -- that of a subset call depends on its list --, the persistent schedule, a failed
    // call) this call waits for all of it; across a capture boundary there is nothing to wait for, the fork orders the two.
    const int guarded = (!call.map && ngroups == 1 && p->last_np == n_packets && p->last_cp == k.cp && enc_pipe_call_set(p, 0, cap) >= 0) ? p->evC_valid : 0;
    p->last_np = n_packets; p->last_cp = k.cp;
    hipError_t lerr = enc_pipe_fork(p, st, cap, true, guarded ? 0 : ENC_END_C, guarded ? 0 : ENC_END_A);
    for (int g = 0; g < ngroups && lerr == hipSuccess; g++) lerr = enc_group_chunks(p, enc_group(p, call, n_packets, g, G), k, g * k.nchunks, guarded);
    // (sC's last launch waits for sB's.)  Chunk-wise hand-over guards only for single-group calls of every stream
    return enc_pipe_join(p, st, cap, p->sC, lerr, (ngroups == 1 && !call.map) ? k.nchunks : 0, k.tm ? ngroups * k.nchunks : (ngroups == 1 ? k.nchunks : 0), k.tm);
}
#undef ENC_TRY
#endif

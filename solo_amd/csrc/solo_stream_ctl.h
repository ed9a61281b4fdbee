// solo_stream_ctl.h -- per-stream control records of solo_batch_reset_streams / solo_recv_reset_streams (include/solo_mi355x.h), and the
// two rules for a caller's list of streams or rows: sx_list_ok for the host lists of the reset and control calls, sx_map_ok /
// sx_map_refused for the lists of subset calls.
//
// The host validates the caller's controls and turns each listed stream into one record; the records travel to the device BY VALUE,
// as the kernel argument of a list launch (up to SX_CTL_PER_LAUNCH records, one workgroup per record).  Nothing is staged in host or
// device memory, so the caller's arrays are free as soon as the call returns and two calls in flight cannot overwrite each other.
#pragma once
#include <stdint.h>
#include <vector>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

struct SxStreamCtl {
    int32_t stream;              // index in the handle
    int32_t a, b, c;             // encoder: SILK rate (bps), useMDIndex, useDTX; decoder: useMDIndex, -, -; receiver ring: first sequence number, -, -
};
#define SX_CTL_PER_LAUNCH 128    // 2 KB of kernel arguments per launch
struct SxStreamCtlList {
    SxStreamCtl r[SX_CTL_PER_LAUNCH];
};

// The HOST list of a reset or control call (streams of a handle, rows of an object): 1 .. n_rows indices inside [0, n_rows), none twice
static inline bool sx_list_ok(const int32_t* rows, int32_t n, int32_t n_rows) {
    if (!rows || n <= 0 || n > n_rows) return false;
    std::vector<char> seen((size_t)n_rows, 0);
    for (int32_t i = 0; i < n; i++) {
        if (rows[i] < 0 || rows[i] >= n_rows || seen[(size_t)rows[i]]) return false;
        seen[(size_t)rows[i]] = 1;
    }
    return true;
}

#if defined(__HIPCC__)
// The one loop behind every list launcher (solo_dec_kernels.h, solo_enc_kernels.h): n records, validated by the caller, go out
// SX_CTL_PER_LAUNCH at a time; launch(l, k) enqueues one launch of k workgroups, one per record of l.  (A callable, not the kernel and
// its arguments: the kernels do not agree on how many arguments stand in front of the list.)
template <typename Launch>
static inline hipError_t sx_launch_ctl_batches(const SxStreamCtl* recs, int n, Launch launch) {
    for (int i0 = 0; i0 < n; i0 += SX_CTL_PER_LAUNCH) {
        const int k = n - i0 < SX_CTL_PER_LAUNCH ? n - i0 : SX_CTL_PER_LAUNCH;
        SxStreamCtlList l = {};
        for (int i = 0; i < k; i++) l.r[i] = recs[i0 + i];
        launch(l, k);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
#endif

// Subset calls (solo_batch_encode_streams, solo_batch_decode_streams, solo_recv_decode_streams): compact position i of a launch works
// on the state of stream map[i]; its inputs and outputs stay at position i.  A NULL map is the identity (every other entry point), and
// the kernels branch on it once, wave-uniformly.  The call's verdict word (solo_api.hip: solo_stream_list_check_kernel) is non-zero when
// the list is not strictly increasing inside [0, N): every kernel of such a call leaves before it touches anything.
// The same rule for the host builds of the stages (tests), which get the list in host memory:
static inline bool sx_map_ok(const int32_t* map, int n, int n_rows) {
    if (map)
        for (int i = 0; i < n; i++)
            if (map[i] < 0 || map[i] >= n_rows || (i > 0 && map[i - 1] >= map[i])) return false;
    return true;
}
#if defined(__HIPCC__)
__device__ __forceinline__ bool sx_map_refused(const int32_t* map, const uint32_t* verdict) {
    return map != nullptr && __builtin_amdgcn_readfirstlane((int)*verdict) != 0;
}
// (s wave-uniform: the stream of a one-wavefront-per-stream kernel)
__device__ __forceinline__ int sx_map_stream(const int32_t* map, int s) { return map ? __builtin_amdgcn_readfirstlane(map[s]) : s; }
#endif

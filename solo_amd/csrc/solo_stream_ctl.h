// solo_stream_ctl.h -- per-stream control records of solo_batch_reset_streams / solo_recv_reset_streams (include/solo_mi355x.h).
//
// The host validates the caller's controls and turns each listed stream into one record; the records travel to the device BY VALUE,
// as the kernel argument of a list launch (up to SX_CTL_PER_LAUNCH records, one workgroup per record).  Nothing is staged in host or
// device memory, so the caller's arrays are free as soon as the call returns and two calls in flight cannot overwrite each other.
#pragma once
#include <stdint.h>

struct SxStreamCtl {
    int32_t stream;              // index in the handle
    int32_t a, b, c;             // encoder: SILK rate (bps), useMDIndex, useDTX; decoder: useMDIndex, -, -; receiver ring: first sequence number, -, -
};
#define SX_CTL_PER_LAUNCH 128    // 2 KB of kernel arguments per launch
struct SxStreamCtlList {
    SxStreamCtl r[SX_CTL_PER_LAUNCH];
};

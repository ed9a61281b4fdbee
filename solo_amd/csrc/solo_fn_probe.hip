// solo_fn_probe.hip -- function-level probe of the LPC / NLSF stage functions (solo_fn_probe.h; tests only): one probe kernel per unit,
// one wavefront per case.  A translation unit of its own: a stage function is compiled for its callers, so a second
// caller beside the product kernels of solo_enc_k.hip would change how THOSE are compiled.
#include <hip/hip_runtime.h>
#include "solo_fn_probe.h"

template <int UNIT>
__global__ void __launch_bounds__(64) SX_K(solo_fn_probe_kernel)(int site, int n_cases, const i32* __restrict__ in, int in_words, i32* __restrict__ out,
                                                                 int out_words) {
    __shared__ SxFnProbeWork w;
    const int c = blockIdx.x;
    if (c >= n_cases) return;
    sx_fn_probe_case<UNIT>(&w, site, in + (size_t)c * in_words, out + (size_t)c * out_words);
}

// -> 0, -1: no such fn / record sizes that are not the fn's / a bad count or pointer, -2: the launch failed
extern "C" int32_t SX_K(solo_fn_probe_launch)(int32_t fn, int32_t n_cases, const int32_t* d_in, int32_t in_words, int32_t* d_out, int32_t out_words,
                                              void* hip_stream) {
    int iw = 0, ow = 0;
    if (!sx_fn_probe_words(fn, &iw, &ow) || iw != in_words || ow != out_words || n_cases < 0 || n_cases > (1 << 16)) return -1;
    if (n_cases == 0) return 0;
    if (!d_in || !d_out) return -1;
    const int unit = fn >> 2, site = fn & 3;
    const hipStream_t s = (hipStream_t)hip_stream;
#define SX_FNP_LAUNCH(U) hipLaunchKernelGGL(SX_K(solo_fn_probe_kernel)<U>, dim3(n_cases), dim3(64), 0, s, site, n_cases, d_in, iw, d_out, ow)
    switch (unit) {
    case SX_FNP_A2NLSF: SX_FNP_LAUNCH(SX_FNP_A2NLSF); break;
    case SX_FNP_NLSF2A: SX_FNP_LAUNCH(SX_FNP_NLSF2A); break;
    case SX_FNP_MSVQ: SX_FNP_LAUNCH(SX_FNP_MSVQ); break;
    case SX_FNP_BURG: SX_FNP_LAUNCH(SX_FNP_BURG); break;
    default: SX_FNP_LAUNCH(SX_FNP_FIND_LPC); break;
    }
#undef SX_FNP_LAUNCH
    if (hipGetLastError() != hipSuccess) return -2;
    return hipStreamSynchronize(s) == hipSuccess ? 0 : -2;
}

#if SX_FS_KHZ == 8
extern "C" int32_t solo_fn_probe_launch_wb(int32_t fn, int32_t n_cases, const int32_t* d_in, int32_t in_words, int32_t* d_out, int32_t out_words, void* hip_stream);
// include/solo_mi355x.h
extern "C" int32_t solo_debug_fn(int32_t samplerate, int32_t fn, int32_t n_cases, const int32_t* d_in, int32_t in_words, int32_t* d_out, int32_t out_words,
                                 void* hip_stream) {
    if (samplerate == 16000) return solo_fn_probe_launch(fn, n_cases, d_in, in_words, d_out, out_words, hip_stream);
    if (samplerate == 32000) return solo_fn_probe_launch_wb(fn, n_cases, d_in, in_words, d_out, out_words, hip_stream);
    return -1;
}
#endif

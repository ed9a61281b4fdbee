// solo_api_wb.hip -- the decoder kernels compiled for the 32 kHz API rate (`samplerate == 32000` in USER_Ctrl_dec,
// libBWE/AGR_BWE_SDK_API.c:197): 16 kHz bands, SILK running wide band (fs_kHz = 16, LPC order 16, order-16 NLSF codebooks,
// stage-3 pitch contours, 320-sample frames), 1280-sample packets.  Same source as the 16 kHz build (solo_dec.h), other
// compile-time constants; a handle whose decoder control asks for this rate holds this build's launch table (solo_dec_ops.h).
#define SX_FS_KHZ 16
#include "solo_dec_kernels.h"

extern "C" const solo_dec_ops* solo_wb_dec_ops() { return &solo_dec_ops_table_wb; }

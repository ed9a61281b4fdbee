// solo_fn_probe_wb.hip -- the function-level probe compiled for the 32 kHz API rate; same source as solo_fn_probe.hip.
#define SX_FS_KHZ 16
#include "solo_fn_probe.hip"

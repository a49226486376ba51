// WARP kernel, plain stores (and the serial mode)
#include "warp_kernels.h"

SMORE_WARP_INST(s, WARP_STORE)

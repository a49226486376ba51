// WARP kernel, plain stores (and the serial mode)
#include "warp_kernels.h"

SMORE_UPDATE_INST(Warp, WARP_STORE, WARP_KMAX, warp_symbol)

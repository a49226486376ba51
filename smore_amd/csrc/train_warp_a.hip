// WARP kernel, atomic scatter
#include "warp_kernels.h"

SMORE_UPDATE_INST(Warp, WARP_ATOMIC, WARP_KMAX, warp_symbol)

// WARP kernel, atomic scatter
#include "warp_kernels.h"

SMORE_WARP_INST(a, WARP_ATOMIC)

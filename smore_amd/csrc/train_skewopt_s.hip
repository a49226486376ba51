// Skew-OPT kernel, plain stores (the serial mode)
#include "skewopt_kernels.h"

SMORE_UPDATE_INST(SkewOpt, MODE_STORE, SKEWOPT_KMAX, skewopt_symbol)

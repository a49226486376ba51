// Skew-OPT kernel, atomic scatter
#include "skewopt_kernels.h"

SMORE_UPDATE_INST(SkewOpt, MODE_ATOMIC, SKEWOPT_KMAX, skewopt_symbol)

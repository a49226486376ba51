// CSE kernels (nemf, nerank), atomic scatter
#include "cse_kernels.h"

SMORE_UPDATE_INST(Cse, MODE_ATOMIC, CSE_NEG, cse_symbol)
SMORE_UPDATE_INST(Cse, MODE_ATOMIC, CSE_RANK_NEG, cse_symbol)

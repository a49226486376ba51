// CSE kernels (nemf, nerank), plain stores (the serial mode)
#include "cse_kernels.h"

SMORE_UPDATE_INST(Cse, MODE_STORE, CSE_NEG, cse_symbol)
SMORE_UPDATE_INST(Cse, MODE_STORE, CSE_RANK_NEG, cse_symbol)

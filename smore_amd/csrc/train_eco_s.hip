// ECO kernels (the sampled-softmax choice rule), plain stores (the serial mode): the three K buckets
#include "eco_kernels.h"

SMORE_UPDATE_INST(Eco, MODE_STORE, 5, eco_symbol)
SMORE_UPDATE_INST(Eco, MODE_STORE, 10, eco_symbol)
SMORE_UPDATE_INST(Eco, MODE_STORE, 20, eco_symbol)

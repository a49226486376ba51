// ECO kernels (the sampled-softmax choice rule), atomic scatter: the three K buckets
#include "eco_kernels.h"

SMORE_UPDATE_INST(Eco, MODE_ATOMIC, 5, eco_symbol)
SMORE_UPDATE_INST(Eco, MODE_ATOMIC, 10, eco_symbol)
SMORE_UPDATE_INST(Eco, MODE_ATOMIC, 20, eco_symbol)

// pair_train_kernel instantiations: atomic scatter, up to 5 negatives (edge_inst.h)
#include "edge_inst.h"
SMORE_UPDATE_INST(Pair, smore::MODE_ATOMIC, 5, pair_symbol)

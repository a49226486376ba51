// pair_train_kernel instantiations: plain-store scatter, up to 10 negatives (edge_inst.h)
#include "edge_inst.h"
SMORE_UPDATE_INST(Pair, smore::MODE_STORE, 10, pair_symbol)

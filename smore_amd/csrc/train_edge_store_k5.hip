// edge_train_kernel instantiations: store scatter, up to 5 negatives (edge_inst.h)
#include "edge_inst.h"
SMORE_UPDATE_INST(Edge, smore::MODE_STORE, 5, edge_symbol)

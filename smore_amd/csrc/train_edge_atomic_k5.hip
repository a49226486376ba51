// edge_train_kernel instantiations: atomic scatter, up to 5 negatives (edge_inst.h)
#include "edge_inst.h"
SMORE_UPDATE_INST(Edge, smore::MODE_ATOMIC, 5, edge_symbol)

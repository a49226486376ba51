// edge_train_kernel instantiations: hybrid scatter, up to 10 negatives (edge_inst.h)
#include "edge_inst.h"
SMORE_UPDATE_INST(Edge, smore::MODE_HYBRID, 10, edge_symbol)

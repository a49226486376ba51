// CBOW kernels (GCN, TEXTGCN), plain stores (the serial mode)
#include "cbow_kernels.h"

SMORE_UPDATE_INST(Cbow, MODE_STORE, CBOW_BATCH, cbow_symbol)

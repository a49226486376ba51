// CBOW kernels (GCN, TEXTGCN), atomic scatter
#include "cbow_kernels.h"

SMORE_UPDATE_INST(Cbow, MODE_ATOMIC, CBOW_BATCH, cbow_symbol)

// HOP-REC kernel, atomic scatter
#include "hoprec_kernels.h"

SMORE_UPDATE_INST(HopRec, MODE_ATOMIC, HOPREC_KMAX, hoprec_symbol)

// HOP-REC kernel, plain stores (the serial mode)
#include "hoprec_kernels.h"

SMORE_UPDATE_INST(HopRec, MODE_STORE, HOPREC_KMAX, hoprec_symbol)

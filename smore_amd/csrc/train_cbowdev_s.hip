// CBOWdev kernels (TEXTGCNdev), plain stores (the serial mode)
#include "cbowdev_kernels.h"

SMORE_UPDATE_INST(CbowDev, MODE_STORE, CBOWDEV_BATCH, cbowdev_symbol)

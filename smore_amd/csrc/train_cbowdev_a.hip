// CBOWdev kernels (TEXTGCNdev), atomic scatter
#include "cbowdev_kernels.h"

SMORE_UPDATE_INST(CbowDev, MODE_ATOMIC, CBOWDEV_BATCH, cbowdev_symbol)

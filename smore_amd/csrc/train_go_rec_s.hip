// go_rec_kernel instantiations (go_rec.h): MODE_STORE scatter, KMAX 5 and 10; the Go walk-pair kernel likewise
#include "go_rec.h"
SMORE_UPDATE_INST(GoRec, smore::MODE_STORE, 5, go_rec_symbol)
SMORE_UPDATE_INST(GoRec, smore::MODE_STORE, 10, go_rec_symbol)
SMORE_UPDATE_INST(GoPair, smore::MODE_STORE, 5, go_pair_symbol)
SMORE_UPDATE_INST(GoPair, smore::MODE_STORE, 10, go_pair_symbol)

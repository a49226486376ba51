// gcn -- the set-sum rule with vertex = context = the source (GCN); see cbow_cli.h
#include "cbow_cli.h"

int main(int argc, char** argv) { return cbow_main(argc, argv, SMORE_CBOW_GCN); }

// nemf -- CSE with the factorisation direct term (NEMF); see cse_cli.h
#include "cse_cli.h"

int main(int argc, char** argv) { return cse_main(argc, argv, 0); }

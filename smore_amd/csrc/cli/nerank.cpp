// nerank -- CSE with the ranking direct term (NERANK); see cse_cli.h
#include "cse_cli.h"

int main(int argc, char** argv) { return cse_main(argc, argv, 1); }

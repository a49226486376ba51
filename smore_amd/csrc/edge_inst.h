// edge_inst.h -- the (G, M) ladders of edge_train_kernel and
// pair_train_kernel: one translation unit per (scatter MODE, KMAX)
// (train_edge_<mode>_k<KMAX>.hip, train_pair_<s|a|h><KMAX>.hip) so the build
// compiles them in parallel.  A unit instantiates its kernels by naming them
// here and exports them as its update_symbol specialisation
// (train_kernels.h SMORE_UPDATE_INST); the resolver and the launch are
// train_kernels.hip's update_kernel and train_kernels.h's launch_update.
#pragma once
#include "edge_kernels.h"

namespace smore {

// by (G, M) and the model's rule (SH = 0: LINE-2's two tables, 1: one shared
// table, LINE-1 / MF, 2: BPR, KMAX 5 only)
template <int KMAX, int MODE>
const void* edge_symbol(int dpad, int model) {
    const int G = lanes_of(dpad), M = regs_of(dpad);
#define X(g, m)                                                                          \
    if (G == g && M == m) {                                                              \
        if (model == SMORE_BPR) {                                                        \
            if constexpr (KMAX == 5) return (const void*)edge_train_kernel<g, m, 5, MODE, 2>; \
            else return nullptr;                                                         \
        }                                                                                \
        return model == SMORE_LINE2 ? (const void*)edge_train_kernel<g, m, KMAX, MODE, 0> \
                                    : (const void*)edge_train_kernel<g, m, KMAX, MODE, 1>; \
    }
    SMORE_FOR_EACH_GM(X)
#undef X
    return nullptr;
}

// DeepWalk pair records in the Hogwild modes (pair_train_kernel)
template <int KMAX, int MODE>
const void* pair_symbol(int dpad, int) {
    const int G = lanes_of(dpad), M = regs_of(dpad);
#define X(g, m) \
    if (G == g && M == m) return (const void*)pair_train_kernel<g, m, KMAX, MODE>;
    SMORE_FOR_EACH_GM(X)
#undef X
    return nullptr;
}

}  // namespace smore

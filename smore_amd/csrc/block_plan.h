// block_plan.h -- the host-only plan of one part's block tables (the 2-D
// block schedule, blocks.cpp): everything smore_block_setup
// derives from the graph and the draw laws before it touches the device.
// Pure host arithmetic over host_graph.h and the standard library (no HIP,
// no environment), so tests/c/block_plan_check.cpp runs the product's plan on
// the CPU.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "host_graph.h"

namespace smore {

// the exact per-draw laws of the graph's alias tables (draw_probabilities)
struct DrawLaws {
    std::vector<double> ps, pn, pc;   // source, negative, marginal context
};

struct BlockPlanArgs {
    bool walk = false;     // walk cells (the C++ walk models); else LINE-2 cells
    int nparts = 2, part = 0;
    int K = 0;
    bool hybrid = false;   // hot tags wanted (the hybrid scatter)
    int64_t H = 0;         // hub C rows, already resolved (blocks.cpp hub_count)
    int64_t M = 0;         // resident sample groups of a cell launch (0 when not hybrid)
    double tau = 0.0;      // a row is hot iff M * p > tau (0 when not hybrid)
    const uint8_t* hot_c = nullptr;   // walk cells, hybrid: the global hot-C flags (V; hot_maps.cpp build_hot_maps)
};

struct BlockPlan {
    // what smore_ctx::Blocks keeps on the host (ctx.h describes each)
    std::vector<int64_t> wb, cb;
    std::vector<double> mass, part_mass, nmass;
    std::vector<uint64_t> atom_off;
    std::vector<int32_t> hubs;
    std::vector<double> hub_rate;
    uint64_t hub_off = 0, nhub = 0;
    std::vector<double> hub_p;
    std::vector<double> pmax_w, pmax_c;
    // the device tables, in their device layout
    hvec<AliasEntry> ntab;              // V: block b's negative alias entries at [cb[b], cb[b + 1])
    std::vector<AliasEntry> hub_ntab;   // nb x H: block k's negative alias entries of the hub slots
    std::vector<int32_t> hub_of;        // walks with hubs: V entries, -1 or the vertex's slot | hot tag << 30
    hvec<uint32_t> atoms;               // LINE-2: 8 words per atom {thr, v, c, 0}, {v', c', 0, 0}
    // per block: the C-row law of its cell over [cb[k], cb[k + 1]) then the H
    // hub slots, and those rows' hot flags (blocks.cpp block_sh_sets)
    std::vector<std::vector<double>> pcb;
    std::vector<std::vector<uint8_t>> hcb;
};

// Part a.part's plan.  Returns "" or the reason the graph cannot be cut this
// way (an empty part or block, a part without edges).
std::string build_block_plan(const HostGraph& g, const DrawLaws& laws, const BlockPlanArgs& a, BlockPlan& p);

}  // namespace smore

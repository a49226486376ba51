// block_plan_check -- the block schedule's host-only plan (smore_amd/csrc/
// block_plan.cpp, the code smore_block_setup runs) on the CPU, its arrays
// written to files for tests/test_block_plan_cpu.py.
//
//   block_plan_check EDGELIST UNDIRECTED MODEL NPARTS PART K H HYBRID M TAU OUTDIR
//
// MODEL: line2 | walk.  H: the resolved hub count.  OUTDIR gets one raw
// little-endian file per array (NAME.bin) and index.txt, one line of
// NAME:TYPE:COUNT entries (pcb / hcb: the blocks' vectors end to end, block k
// holding cb[k + 1] - cb[k] + H entries).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../smore_amd/csrc/block_plan.h"

using namespace smore;

static std::string g_dir, g_index;

template <class T>
static bool put(const char* name, const char* type, const T* data, size_t n) {
    const std::string path = g_dir + "/" + name + ".bin";
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = n == 0 || fwrite(data, sizeof(T), n, f) == n;
    g_index += std::string(name) + ":" + type + ":" + std::to_string(n) + " ";
    return fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
    if (argc != 12) {
        fprintf(stderr, "usage: %s EDGELIST UNDIRECTED line2|walk NPARTS PART K H HYBRID M TAU OUTDIR\n", argv[0]);
        return 2;
    }
    BlockPlanArgs a;
    a.walk = !strcmp(argv[3], "walk");
    a.nparts = atoi(argv[4]);
    a.part = atoi(argv[5]);
    a.K = atoi(argv[6]);
    a.H = atoll(argv[7]);
    a.hybrid = atoi(argv[8]) != 0;
    a.M = atoll(argv[9]);
    a.tau = atof(argv[10]);
    g_dir = argv[11];
    if ((!a.walk && strcmp(argv[3], "line2")) || a.nparts < 2 || a.part < 0 || a.part >= a.nparts || a.K < 0 || a.H < 0) {
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    if (a.walk && a.hybrid) {   // their C tags are the device path's hot maps (hot_maps.cpp build_hot_maps)
        fprintf(stderr, "walk cells: not hybrid here\n");
        return 2;
    }
    std::vector<std::string> names;
    std::vector<int32_t> src, dst;
    std::vector<double> w;
    std::string err;
    HostGraph g;
    if (!read_edgelist(argv[1], atoi(argv[2]) != 0, names, src, dst, w, err) ||
        !build_graph((int64_t)names.size(), (int64_t)src.size(), src.data(), dst.data(), w.data(), 0, 0, g, err)) {
        fprintf(stderr, "graph: %s\n", err.c_str());
        return 1;
    }
    if (g.V < 2 * a.nparts || a.H > g.V / 2) {
        fprintf(stderr, "graph too small for the parts / hubs\n");
        return 2;
    }
    DrawLaws laws;
    draw_probabilities(g, laws.ps, laws.pn, laws.pc);
    BlockPlan p;
    err = build_block_plan(g, laws, a, p);
    if (!err.empty()) {
        fprintf(stderr, "%s\n", err.c_str());
        return 1;
    }
    const uint64_t hub_range[2] = {p.hub_off, p.nhub};
    std::vector<double> pcb;
    std::vector<uint8_t> hcb;
    for (size_t k = 0; k < p.pcb.size(); ++k) {
        pcb.insert(pcb.end(), p.pcb[k].begin(), p.pcb[k].end());
        hcb.insert(hcb.end(), p.hcb[k].begin(), p.hcb[k].end());
    }
    bool ok = put("wb", "i64", p.wb.data(), p.wb.size()) && put("cb", "i64", p.cb.data(), p.cb.size()) &&
              put("mass", "f64", p.mass.data(), p.mass.size()) &&
              put("part_mass", "f64", p.part_mass.data(), p.part_mass.size()) &&
              put("nmass", "f64", p.nmass.data(), p.nmass.size()) &&
              put("atom_off", "u64", p.atom_off.data(), p.atom_off.size()) &&
              put("hubs", "i32", p.hubs.data(), p.hubs.size()) &&
              put("hub_rate", "f64", p.hub_rate.data(), p.hub_rate.size()) && put("hub_range", "u64", hub_range, 2) &&
              put("hub_p", "f64", p.hub_p.data(), p.hub_p.size()) &&
              put("pmax_w", "f64", p.pmax_w.data(), p.pmax_w.size()) &&
              put("pmax_c", "f64", p.pmax_c.data(), p.pmax_c.size()) &&
              put("ntab", "u32", reinterpret_cast<const uint32_t*>(p.ntab.data()), 2 * p.ntab.size()) &&
              put("hub_ntab", "u32", reinterpret_cast<const uint32_t*>(p.hub_ntab.data()), 2 * p.hub_ntab.size()) &&
              put("hub_of", "i32", p.hub_of.data(), p.hub_of.size()) &&
              put("atoms", "u32", p.atoms.data(), p.atoms.size()) && put("pcb", "f64", pcb.data(), pcb.size()) &&
              put("hcb", "u8", hcb.data(), hcb.size());
    FILE* f = ok ? fopen((g_dir + "/index.txt").c_str(), "w") : nullptr;
    if (!f || fprintf(f, "%s\n", g_index.c_str()) < 0 || fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", g_dir.c_str());
        return 1;
    }
    return 0;
}

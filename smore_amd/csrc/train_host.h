// train_host.h -- what the host translation units of the C ABI share beyond
// the context (ctx.h): the source partition and the hot-row / write-combine
// policy (hot_maps.cpp), the record-launch path of the training drivers
// (train.cpp) and the caller-pairs core (train.cpp, used by pairs_rows.cpp).
// Internal: not part of the installed interface.
#pragma once
#include <utility>

#include "ctx.h"
#include "go_walks.h"

namespace smore_host {

inline int check_table(smore_ctx* c, int which) {
    if (!c) return SMORE_EINVAL;
    if (which < 0 || which >= c->ntables || !c->d_table[which]) return fail(c, SMORE_ESTATE, "table not allocated");
    return SMORE_OK;
}

// a device buffer of at least `need` elements: grown to exactly `need` (the
// old one freed first -- hipFree waits for the device -- so the footprint
// never holds both)
template <class T>
int ensure_cap(smore_ctx* c, T*& p, size_t& cap, size_t need) {
    if (cap >= need) return SMORE_OK;
    dfree(p);
    cap = 0;
    HIPCHK(c, hipMalloc((void**)&p, need * sizeof(T)));
    cap = need;
    return SMORE_OK;
}

// ---------------------------------------------------------------- hot_maps.cpp
int apply_partition(smore_ctx* c);

// the 2-D block schedule's per-cell concurrency cap (blocks.cpp cell_grid):
// at most this many updates per round on a cell's hottest row (0: no cap).
// Walk cells need it: C5 DeepWalk on 8 GPUs (top row M p = 2048 per round)
// diverged without it and reached 1.027 x the one-GPU held-out loss with 512
// (1024: 1.027, 256: 1.024).  LINE-2 cells do not: C2 on 8 GPUs with the
// atomic scatter is at 0.99 x one GPU uncapped; what the hybrid loses there is
// the cold rows' plain stores (HOT_TAU_CELL), and the cap costs the hub cells
// 1.5-3 x (C4, 8 GPUs: predicted speed-up 3.4 x capped vs 4.9 x)
constexpr double CELL_RATE_PAIRS = 512.0, CELL_RATE_EDGES = 0.0;

// hot-row threshold defaults (smore_set_hot_threshold(ctx, -1)): the C++
// rules' edge-record kernel takes 1.0 (C4 / C2 update 4 % / 12 % faster than
// at 0.3, held-out loss +0.1 / +0.2 % of the atomic scatter's); the Go edge
// rules (no faster at 1.0: C4 Go LINE-2 1140 vs 1133 M/s) and the pair-record
// kernels keep 0.3 (on small graphs the walk models' runs of W_v updates need
// the context rows' atomics: Go DeepWalk AUC on the 920-vertex graph 0.881 at
// 1.0 vs 0.900 at 0.3, serial 0.906); DESIGN.md 8, profiles/r03/tau
constexpr double HOT_TAU_EDGE = 1.0, HOT_TAU_WALK = 0.3;
// LINE-2 cells of the 2-D block schedule: a cell's law is its C block's
// (1/2N of the rows) renormalised, so more of its updates land on rows just
// under the threshold, where plain stores collide.  C2 LINE-2 held-out loss
// on 8 GPUs / one GPU: tau 1.0 1.065, 0.5 1.026, 0.3 1.020 (atomic 0.99);
// C4 8-GPU predicted speed-up 4.9 x at 0.3 and 0.5 (profiles/r05/blocks.md)
constexpr double HOT_TAU_CELL = 0.3;

// PAIR_FLUSH_MAX: the pair-record kernels' automatic drain interval (8 rounds,
// the floor, instead of up to 32): a group runs a walk's consecutive records,
// so a combined context row gathers its pending deltas in bursts; C5 DeepWalk
// (d=128, 10 walks per vertex) held-out loss / AUC: drain 32 rounds (the edge
// rule's choice there) 0.5648 / 0.9835 in 2.99 s, 16: 0.5444 / 0.9840 in 3.02
// s, 8: 0.5376 / 0.9847 in 3.20 s, no combining 0.5312 / 0.9843 in 4.28 s,
// atomic 0.5276 / 0.9844 in 6.98 s (profiles/r04/walk_combine.jsonl)
constexpr int EDGE_FLUSH_MAX = 32, PAIR_FLUSH_MAX = 8;

// the hidden-update budget of a cell's write-combined rows and the staleness
// bound of the edge (false) / pair (true) rule; SMORE_SH_BUDGET / SMORE_SH_STALE
// override (hot_maps.cpp, with the constants)
double cell_budget(bool walk);
double sh_stale(bool pairs);
int slot_interval(double Mp, int cap, double budget);
void sh_levels(int64_t M, int cap, double budget, const std::pair<double, int32_t>* r, int64_t n, int (&lvl)[8]);
int build_hot_maps(smore_ctx* c, int model, int K, int64_t M, double tau_default, int flush_max = EDGE_FLUSH_MAX,
                   double w_scale = 1.0, double c_scale = 1.0);
int ensure_packed(smore_ctx* c);

// train_hoprec.cpp: a field-0 vertex can come out of SourceSample (HOP-REC and CSE start there)
bool field0_has_source_mass(const smore_ctx* c);

// ---------------------------------------------------------------- train.cpp
// the grid of an update launch of up to `count` records through kernel k
// (train_kernels.h update_kernel) in scatter `mode`: what the occupancy of k
// allows, under the knobs' and the small-graph caps
int edge_grid(smore_ctx* c, const UpdateKernel& k, int mode, uint64_t count, bool leave_slot = false);
inline int edge_grid(smore_ctx* c, UpdateFamily f, const EdgeArgs& a, bool leave_slot = false) {
    return edge_grid(c, update_kernel(f, a), a.mode, a.count, leave_slot);
}
int grow_events(smore_ctx* c, std::vector<hipEvent_t>& v, size_t n);
// the update-kernel arguments every record path fills alike (the tables by
// the model's row roles); the caller adds its own
EdgeArgs record_args(smore_ctx* c, int model, int K, int mode);
// the launch plan of a record path whose a.count bounds a chunk's records:
// the grid (LDS sized for the most write-combined rows), the hot maps of a
// hybrid launch for that grid, then the write-combined set they chose in a
int plan_record_launch(smore_ctx* c, EdgeArgs& a, bool combine, UpdateFamily f, int hot_model, double tau_default,
                       int flush_max, int* grid);
// the plan of the drivers whose records are LINE-2 pairs with the rate in the
// record (walks, APP, HPE, caller pairs): the arguments (at most max_records
// per chunk, in c->d_rec, sized by the caller before) and the grid, the
// tables as the hot maps left them
int plan_pair_records(smore_ctx* c, UpdateFamily f, int K, int mode, uint64_t total, uint64_t seed, double alpha0,
                      double reg, uint64_t max_records, EdgeArgs* a, int* grid);
// one chunk of pair records through the family's update kernel of the mode
// (the row census instead while one is in progress)
int launch_record_update(smore_ctx* c, UpdateFamily f, const EdgeArgs& ak, int grid);
int finish_timed(smore_ctx* c, int mode, int phase_n);
// a blocking wrapper's tail: the async call's rc, or the stream's completion
int sync_after(smore_ctx* c, int rc, bool check_last_error = false);
// smore_train_pairs queued on the stream (the caller synchronizes)
int train_pairs_core(smore_ctx* c, const int32_t* v, const int32_t* cc, int64_t n, int K, double alpha, uint64_t seed,
                     uint64_t unit, int mode);

}  // namespace smore_host

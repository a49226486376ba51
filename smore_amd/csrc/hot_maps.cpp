// hot_maps.cpp -- which rows a launch treats specially: the source partition
// of a replica, and the hybrid scatter's hot-row tags and write-combined set
//  with the constants that decide them.
#include "train_host.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace smore_host;

namespace smore_host {

// ---------------------------------------------------------------- source partition
// the source law restricted to part i of n and renormalised
static void partition_law(const std::vector<double>& ps, int n, int i, std::vector<double>& law) {
    std::vector<int64_t> bound;
    source_bounds(ps, n, bound);
    law.assign(ps.size(), 0.0);
    double sum = 0.0;
    for (int64_t v = bound[i]; v < bound[i + 1]; ++v) sum += ps[v];
    if (sum > 0.0)
        for (int64_t v = bound[i]; v < bound[i + 1]; ++v) law[v] = ps[v] / sum;
}

// Restrict the device vertex table to this context's part (renormalised, Go
// alias rule with power 1: any valid encoding of the law; N > 1 only, where
// draws are not compared with one GPU's) and upload it.
int apply_partition(smore_ctx* c) {
    const HostGraph& g = *c->g;
    int rc;
    if ((rc = set_device(c))) return rc;
    c->packed_ok = false;
    c->hot_key.clear();
    if (c->part_n <= 1) {
        c->part_vtab.clear();
        c->part_bounds.clear();
        return upload(c, c->d_vtab, g.vtab.data(), g.vtab.size());
    }
    std::vector<double> ps, pn, pc;
    draw_probabilities(g, ps, pn, pc);
    std::vector<int64_t>& bound = c->part_bounds;
    source_bounds(ps, c->part_n, bound);
    const int64_t lo = bound[c->part_i], hi = bound[c->part_i + 1];
    if (hi <= lo) return fail(c, SMORE_EINVAL, "source partition: an empty part (more parts than vertices with mass)");
    std::vector<double> w((size_t)g.V, 0.0), prob((size_t)g.V);
    std::vector<int64_t> alias((size_t)g.V);
    for (int64_t v = lo; v < hi; ++v) w[v] = ps[v];
    alias_go(w.data(), g.V, 1.0, prob.data(), alias.data());
    c->part_vtab.resize((size_t)g.V);
    alias_encode(prob.data(), alias.data(), g.V, nullptr, c->part_vtab.data());
    return upload(c, c->d_vtab, c->part_vtab.data(), c->part_vtab.size());
}

}  // namespace smore_host

extern "C" {

int smore_source_parts(smore_ctx* c, int nparts, int64_t* bounds) {
    if (!c || !bounds || nparts < 1) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (nparts > c->g->V) return fail(c, SMORE_EINVAL, "more parts than vertices");
    if (c->part_n == nparts && (int)c->part_bounds.size() == nparts + 1) {   // the active partition's
        std::copy(c->part_bounds.begin(), c->part_bounds.end(), bounds);
        return SMORE_OK;
    }
    std::vector<double> ps, pn, pc;
    draw_probabilities(*c->g, ps, pn, pc);
    std::vector<int64_t> bound;
    source_bounds(ps, nparts, bound);
    std::copy(bound.begin(), bound.end(), bounds);
    return SMORE_OK;
}

int smore_set_source_partition(smore_ctx* c, int nparts, int part) {
    if (!c || nparts < 1 || part < 0 || part >= nparts) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (nparts > c->g->V) return fail(c, SMORE_EINVAL, "more parts than vertices");
    if (c->device < 0) return fail(c, SMORE_ESTATE, "host-only context");
    if (c->part_n == nparts && c->part_i == part) return SMORE_OK;   // kept current by the table setters
    c->part_n = nparts;
    c->part_i = part;
    return apply_partition(c);
}

}  // extern "C"

namespace smore_host {

// ---------------------------------------------------------------- hybrid scatter
// A row is "hot" when the expected number of resident sample groups touching
// it at once, M * p(row), exceeds tau; hot rows take float atomics, the rest
// plain stores (DESIGN.md "Scatter modes").
// Hybrid scatter: rows whose expected number of concurrent updates M * p(row)
// exceeds tau are tagged hot in the device graph's id words (device_common.h):
// W-rows through the vertex table, C-rows through the negative and context
// tables and the CSR targets (one union set for shared-table models).  Written
// in place into the existing device arrays; the host graph stays untagged.
constexpr double SH_STALE_MAX = 65536.0;
// automatic drain interval (smore_set_write_combine flush_rounds 0, the
// default): the hottest combined row gathers about M * p_top * flush updates
// that other workgroups cannot see yet; flush = budget / (M * p_top) within
// [8, 32] rounds keeps that at the config-4 level (flush 32) on hotter graphs
constexpr double SH_AUTO_BUDGET = 6144.0;
// the pair-record kernels' budget (and staleness bound): 1024 hidden updates,
// the one-GPU C5 DeepWalk top row's at its 8-round drain.  A walk group runs
// a walk's records in order, so a hub context row's hidden updates come in
// correlated bursts; 4096 (drain 32 at one GPU) cost C5 held-out loss +6 %,
// and under the 2-D block schedule (a cell's rows nb times hotter: the top
// row M p = 512 per round at 2 GPUs) it diverged (loss 2.6e8; budget 1024:
// 0.5308, one GPU 0.5309; profiles/r05/walk_blocks.txt)
constexpr double SH_PAIR_BUDGET = 1024.0;
static double sh_budget(bool pairs) {
    if (const char* e = getenv("SMORE_SH_BUDGET")) return atof(e);
    return pairs ? SH_PAIR_BUDGET : SH_AUTO_BUDGET;
}
// LINE-2 cells of the 2-D block schedule (blocks.cpp block_sh_sets): twice the
// edge budget.  A cell's hub rows are 2N times hotter, so at the edge budget
// they drain every 1-2 rounds and the hub cells are bound by those drains'
// memory-side atomics; C4 on 8 GPUs predicted 4.9 x at 6144, 5.5 x at 9216,
// 5.8 x at 12288, 6.3 x at 24576, for C2 held-out loss 1.019 / 1.031 / 1.037 /
// 1.077 x one GPU (profiles/r05/blocks)
constexpr double SH_CELL_BUDGET = 12288.0;
double cell_budget(bool walk) {
    if (const char* e = getenv("SMORE_SH_BUDGET")) return atof(e);
    return walk ? SH_PAIR_BUDGET : SH_CELL_BUDGET;
}
// rows whose hidden updates would pass this even at a 1-round drain (edge
// rule) / the budget (pair rule) stay on atomics; SMORE_SH_STALE overrides
double sh_stale(bool pairs) {
    if (const char* e = getenv("SMORE_SH_STALE")) return atof(e);
    return pairs ? SH_PAIR_BUDGET : SH_STALE_MAX;
}

// The thresholds, the drain-interval caps and the cell rates that the drivers
// and the block schedule name (HOT_TAU_*, *_FLUSH_MAX, CELL_RATE_*) are in
// train_host.h, with their measurements.

// w_scale / c_scale (the 2-D block schedule, blocks.cpp): a launch then
// draws its W rows from one part of N and its C rows from one block of 2N, so
// the rows it touches are about N / 2N times as likely per sample as under
// the global law; the tags and the write-combined set follow the scaled law.
// The C-row law and the flags are kept on the host (hot_pc, hot_c) for the
// block tables' own tags and write-combined sets.
// drain interval of one write-combined row with M * p expected updates per
// round: the budget of hidden updates over that rate, a power of two in
// [1, cap] (cap a power of two) -- the two-tier drain's unit
int slot_interval(double Mp, int cap, double budget) {
    int f = 1;
    while (2 * f <= cap && (double)(2 * f) * Mp <= budget) f *= 2;
    return f;
}

// EdgeArgs::sh_lvl of n slots sorted by rate: lvl[j] = the slots whose own
// interval is at most 2^j (and below cap, which every slot drains at)
void sh_levels(int64_t M, int cap, double budget, const std::pair<double, int32_t>* r, int64_t n, int (&lvl)[8]) {
    for (int j = 0; j < 8; ++j) {
        int64_t k = 0;
        while (k < n && slot_interval((double)M * r[k].first, cap, budget) <= (1 << j) && (1 << j) < cap) ++k;
        lvl[j] = (int)k;
    }
}

int build_hot_maps(smore_ctx* c, int model, int K, int64_t M, double tau_default, int flush_max, double w_scale,
                   double c_scale) {
    // Small graphs (the V/16 concurrency cap binds: 16 M >= V, e.g. the test
    // graphs, never C2-C5): with the default threshold every touched row is
    // hot and nothing is write-combined, i.e. the hybrid is the lossless
    // atomic scatter.  There every row is a hub (920 vertices: M p ~ 0.3-3 for
    // most rows), plain stores lose updates at any threshold (caller pairs,
    // C++ rules: held-out loss +2.6 % at tau 0.3, +16 % at 1.0, atomic +0.06 %;
    // profiles/r04/pairs_probe.jsonl), and the tables sit in L2, so the
    // memory-side traffic the hybrid saves does not exist.  An explicit
    // smore_set_hot_threshold keeps its meaning.
    const bool small = c->hot_tau < 0 && 16.0 * (double)M >= (double)c->g->V;
    const double tau = c->hot_tau >= 0 ? c->hot_tau : small ? 0.0 : tau_default;
    char key[128];
    const char* stale_env = getenv("SMORE_SH_STALE");
    // W rows of two-table models stay out of the write-combined set unless
    // SMORE_SH_WROWS=1: combining the hub W rows makes their pending deltas
    // invisible for a whole drain window, which cost Go LINE-2 (source law
    // out_degree^1, ~1 % of samples on one W row) 4.7 % held-out loss at C2
    // (0.7 % without), for +12 % C4 throughput; C++ LINE-2 gains nothing from
    // it (1338 vs 1342 M/s), DESIGN.md 8
    const char* wrows_env = getenv("SMORE_SH_WROWS");
    const bool wrows = wrows_env && atoi(wrows_env) != 0;
    // combined W rows drain on their own interval (SMORE_SH_WFLUSH rounds,
    // default 8; 0 = with the context rows)
    const char* wflush_env = getenv("SMORE_SH_WFLUSH");
    const int wflush = wrows ? (wflush_env ? std::max(0, atoi(wflush_env)) : 8) : 0;
    // per-slot drain levels (EdgeArgs::sh_lvl): the C++ rules' edge and pair
    // kernels; the Go record kernels drain on one interval
    const bool two_tier = c->semantics != SMORE_SEM_GO && c->sh_flush <= 0 && !wrows;
    snprintf(key, sizeof key, "%d/%d/%lld/%.9g/%d/%d/%s/%d/%d/%d/%d/%d/%g/%g/%d", model, K, (long long)M, tau,
             c->sh_max, c->sh_flush, stale_env ? stale_env : "", (int)wrows, c->part_n, c->part_i, flush_max, wflush,
             w_scale, c_scale, (int)two_tier);
    if (c->hot_key == key) return SMORE_OK;
    if (c->g->V >= ((int64_t)1 << 30)) return fail(c, SMORE_EINVAL, "hybrid scatter needs V < 2^30");
    std::vector<double> ps, pn, pc;
    draw_probabilities(*c->g, ps, pn, pc);
    if (c->part_n > 1) {
        // this replica draws its sources from its part only: the hot rows
        // follow the restricted law (its part's W rows N times as hot)
        std::vector<double> law;
        partition_law(ps, c->part_n, c->part_i, law);
        draw_probabilities(*c->g, ps, pn, pc, &law);
    }
    const int64_t V = c->g->V, E = c->g->E;
    std::vector<uint8_t> hw((size_t)V, 0), hc((size_t)V, 0);
    const int negs = model == SMORE_BPR ? 5 : K;
    c->hot_rows[0] = c->hot_rows[1] = 0;
    for (int64_t v = 0; v < V; ++v) {
        double pw, pcx;
        if (model == SMORE_LINE2) { pw = ps[v] * w_scale; pcx = (pc[v] + negs * pn[v]) * c_scale; }
        else { pw = pcx = ps[v] + pc[v] + negs * pn[v]; }
        if ((double)M * pw > tau) { hw[v] = 1; c->hot_rows[0]++; }
        if ((double)M * pcx > tau) { hc[v] = 1; c->hot_rows[1]++; }
    }
    // super-hot rows: the hottest hot context rows, write-combined per block
    {
        // the pair-record kernels (walks) pass PAIR_FLUSH_MAX: their budget
        const bool pairs = flush_max == PAIR_FLUSH_MAX;
        const double stale_max = sh_stale(pairs), budget = sh_budget(pairs);
        std::vector<std::pair<double, int32_t>> r;
        const int flush_cap = c->sh_flush > 0 ? c->sh_flush : flush_max;
        for (int64_t v = 0; v < V; ++v) {
            const double p = model == SMORE_LINE2 ? (pc[v] + negs * pn[v]) * c_scale : ps[v] + pc[v] + negs * pn[v];
            // bounded staleness: a combined row's pending deltas are invisible to
            // other workgroups for up to sh_flush rounds, i.e. about
            // M * p * sh_flush updates; rows above SH_STALE_MAX stay on atomics
            // (on small graphs that is every hot row)
            // (two tiers: each row at its own interval, slot_interval)
            const double f = two_tier ? (double)slot_interval((double)M * p, flush_cap, budget) : (double)flush_cap;
            if (hc[v] && (double)M * p * f <= stale_max) r.push_back({p, (int32_t)v});
            // two tables (SMORE_SH_WROWS=1 only): the hub W rows compete for
            // the same slots (key v | SH_WKEY)
            if (wrows && model == SMORE_LINE2 && hw[v] &&
                (double)M * ps[v] * w_scale * (wflush ? wflush : flush_cap) <= stale_max)
                r.push_back({ps[v] * w_scale, (int32_t)(v | SH_WKEY)});
        }
        const int64_t cap =
            small ? 0 : std::max<int64_t>(0, std::min<int64_t>(c->sh_max, sh_rows_max(c->dpad)));
        const int64_t n = std::min<int64_t>(cap, (int64_t)r.size());
        std::partial_sort(r.begin(), r.begin() + n, r.end(), [](const auto& x, const auto& y) {
            return x.first > y.first || (x.first == y.first && x.second < y.second);
        });
        std::vector<int2> hash(SH_HASH, make_int2(-1, -1));
        std::vector<int32_t> ids((size_t)std::max<int64_t>(n, 1), -1);
        for (int64_t i = 0; i < n; ++i) {
            const int32_t id = r[i].second;
            ids[i] = id;
            uint32_t p = sh_hash_of(id);
            while (hash[p & (SH_HASH - 1)].x >= 0) ++p;
            hash[p & (SH_HASH - 1)] = make_int2(id, (int)i);
        }
        int rc2;
        if ((rc2 = set_device(c))) return rc2;
        if ((rc2 = upload(c, c->d_sh_hash, hash.data(), hash.size()))) return rc2;
        if ((rc2 = upload(c, c->d_sh_ids, ids.data(), ids.size()))) return rc2;
        c->sh_rows = (int)n;
        c->sh_flush_eff = flush_cap;
        c->sh_flush_w_eff = wflush;
        // every slot drains every flush_cap rounds; a slot whose own interval
        // (slot_interval) is shorter also at its own (a prefix per level: r is
        // sorted by rate)
        for (int& x : c->sh_lvl_eff) x = 0;
        if (two_tier) sh_levels(M, flush_cap, budget, r.data(), n, c->sh_lvl_eff);
        if (getenv("SMORE_SH_DEBUG")) {
            const int* l = c->sh_lvl_eff;
            fprintf(stderr, "[sh] global M %lld rows %lld of %zu flush %d lvl %d %d %d %d %d %d %d %d top", (long long)M,
                    (long long)n, r.size(), flush_cap, l[0], l[1], l[2], l[3], l[4], l[5], l[6], l[7]);
            for (int64_t i = 0; i < std::min<int64_t>(n, 4); ++i)
                fprintf(stderr, " %d:%.3g", r[i].second, (double)M * r[i].first);
            fprintf(stderr, "\n");
        }
        // the automatic interval follows the hottest row drained on it (with
        // their own interval, W rows do not count)
        int64_t top = 0;
        while (top < n && wflush && (r[top].second & SH_WKEY)) ++top;
        if (c->sh_flush <= 0 && top < n && !two_tier) {
            const double f = budget / ((double)M * r[top].first);
            c->sh_flush_eff = (int)std::max(8.0, std::min((double)flush_cap, std::floor(f)));
        }
    }
    const HostGraph& g = *c->g;
    auto tag_tab = [&](const hvec<AliasEntry>& tab, const std::vector<uint8_t>& hot) {
        std::vector<AliasEntry> t(tab.begin(), tab.end());
        for (int64_t i = 0; i < V; ++i) {
            const uint32_t al = (uint32_t)t[i].alias;
            t[i].alias = (int32_t)(al | ((uint32_t)hot[al] << 30) | ((uint32_t)hot[i] << 31));
        }
        return t;
    };
    int rc;
    if ((rc = set_device(c))) return rc;
    {
        const std::vector<AliasEntry> vt = tag_tab(c->part_n > 1 ? c->part_vtab : g.vtab, hw),
                                      nt = tag_tab(g.ntab, hc);
        HIPCHK(c, hipMemcpy(c->d_vtab, vt.data(), V * sizeof(AliasEntry), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_ntab, nt.data(), V * sizeof(AliasEntry), hipMemcpyHostToDevice));
    }
    // targets and context alias words, in slices to bound the host copy
    const int64_t slice = (int64_t)1 << 26;
    std::vector<int32_t> tt;
    std::vector<AliasEntry> ct;
    for (int64_t b = 0; b < E; b += slice) {
        const int64_t n = std::min(slice, E - b);
        tt.resize((size_t)n);
        ct.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            const int32_t t = g.targets[b + i];
            tt[i] = t | ((int32_t)hc[t] << 30);
            const AliasEntry e = g.ctab[b + i];
            ct[i] = {e.thresh, e.alias | ((int32_t)hc[e.alias] << 30)};
        }
        HIPCHK(c, hipMemcpy(c->d_targets + b, tt.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_ctab + b, ct.data(), n * sizeof(AliasEntry), hipMemcpyHostToDevice));
    }
    c->hot_key = key;
    c->packed_ok = false;
    // the C-row law and flags for the block tables (blocks.cpp)
    c->hot_c.assign(hc.begin(), hc.end());
    c->hot_w.assign(hw.begin(), hw.end());
    c->hot_pc.resize((size_t)V);
    for (int64_t v = 0; v < V; ++v)
        c->hot_pc[v] = model == SMORE_LINE2 ? (pc[v] + negs * pn[v]) * c_scale : ps[v] + pc[v] + negs * pn[v];
    c->hot_M = M;
    c->hot_small = small;
    return SMORE_OK;
}

// packed draw tables (DevGraph::vt32 / ct16): built on the device from the
// current (tagged) tables; skipped when offsets do not fit 32 bits
int ensure_packed(smore_ctx* c) {
    if (c->packed_ok) return SMORE_OK;
    const int64_t V = c->g->V, E = c->g->E;
    if (E >= ((int64_t)1 << 32)) return SMORE_OK;
    if (!c->d_vt32) HIPCHK(c, draw_malloc((void**)&c->d_vt32, (size_t)std::max<int64_t>(V, 1) * 2 * sizeof(uint4)));
    if (!c->d_ct16) HIPCHK(c, draw_malloc((void**)&c->d_ct16, (size_t)std::max<int64_t>(E, 1) * sizeof(uint4)));
    HIPCHK(c, launch_pack(dev_graph(c), (uint64_t)E, c->d_vt32, c->d_ct16, c->stream));
    c->packed_ok = true;
    return SMORE_OK;
}

}  // namespace smore_host

extern "C" {

int smore_set_hot_threshold(smore_ctx* c, double tau) {
    if (!c || tau != tau) return SMORE_EINVAL;
    if (int rc_ = refuse_cse(c)) return rc_;
    if (tau < 0) tau = -1.0;   // the per-path defaults
    c->hot_tau = tau;
    return SMORE_OK;
}

int smore_set_write_combine(smore_ctx* c, int rows, int flush_rounds) {
    if (!c || rows < 0 || rows > 1024 || flush_rounds < 0) return SMORE_EINVAL;
    if (int rc_ = refuse_cse(c)) return rc_;
    c->sh_max = rows;
    c->sh_flush = flush_rounds;
    c->hot_key.clear();
    return SMORE_OK;
}

int smore_write_combine_info(const smore_ctx* c, int* rows, int* flush_rounds) {
    if (!c) return SMORE_EINVAL;
    if (rows) *rows = c->sh_rows;
    if (flush_rounds) *flush_rounds = c->sh_flush_eff;
    return SMORE_OK;
}

// the n rows of table `which` (0: W, 1: C) with the highest expected touches
// per sample under the context's samplers and the model's row roles (LINE-2 /
// Go BPR: W = sources, C = contexts + K x negatives; one-table models: the
// union), highest first -- the rows the replica exchange syncs every launch
int smore_row_rates(smore_ctx* c, int model, int K, int which, int64_t n, double* rate) {
    if (!c || !rate || which < 0 || which > 1 || ((model < 0 || model > 3) && model != SMORE_CENSUS) || K < 0)
        return SMORE_EINVAL;
    if (int rc_ = refuse_cse(c)) return rc_;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    const int64_t V = c->g->V;
    if (n != V) return fail(c, SMORE_EINVAL, "row_rates: n must be the vertex count");
    if (model == SMORE_CENSUS) {
        if (!c->census_ok || (int64_t)c->census_rate[which].size() != V)
            return fail(c, SMORE_ESTATE, "row_rates: no census (smore_census_begin / _end)");
        std::copy(c->census_rate[which].begin(), c->census_rate[which].end(), rate);
        return SMORE_OK;
    }
    std::vector<double> ps, pn, pc;
    draw_probabilities(*c->g, ps, pn, pc);
    const bool two = model == SMORE_LINE2 || (model == SMORE_BPR && c->semantics == SMORE_SEM_GO);
    const int negs = model == SMORE_BPR ? (c->semantics == SMORE_SEM_GO ? 1 : 5) : K;
    for (int64_t v = 0; v < V; ++v)
        rate[v] = two ? (which == 0 ? ps[v] : pc[v] + negs * pn[v]) : ps[v] + pc[v] + negs * pn[v];
    return SMORE_OK;
}

int smore_hot_row_ids(smore_ctx* c, int model, int K, int which, int64_t n, int32_t* ids) {
    if (!c || !ids || n < 0 || which < 0 || which > 1 || ((model < 0 || model > 3) && model != SMORE_CENSUS) || K < 0)
        return SMORE_EINVAL;
    if (int rc_ = refuse_cse(c)) return rc_;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    const int64_t V = c->g->V;
    if (n > V) return fail(c, SMORE_EINVAL, "more hot rows than vertices");
    std::vector<double> rate((size_t)V);
    int rc;
    if ((rc = smore_row_rates(c, model, K, which, V, rate.data()))) return rc;
    std::vector<int32_t> order((size_t)V);
    for (int64_t v = 0; v < V; ++v) order[v] = (int32_t)v;
    std::partial_sort(order.begin(), order.begin() + n, order.end(), [&](int32_t a, int32_t b) {
        return rate[a] > rate[b] || (rate[a] == rate[b] && a < b);
    });
    std::copy(order.begin(), order.begin() + n, ids);
    return SMORE_OK;
}

int smore_hot_rows(const smore_ctx* c, int64_t* hot_w, int64_t* hot_c) {
    if (!c) return SMORE_EINVAL;
    if (hot_w) *hot_w = c->hot_rows[0];
    if (hot_c) *hot_c = c->hot_rows[1];
    return SMORE_OK;
}

}  // extern "C"

// blocks.cpp -- the 2-D block schedule of the multi-GPU path (SURVEY.md 8e's
// conflict-free fallback), one context's side: its draw tables,
// its cell launches and, for the walk models, its bucketed round records.
//
// The reference trains one shared table pair with Hogwild threads
// (src/model/LINE.cpp:160-191, src/model/DeepWalk.cpp:128-155).  Replicated
// tables over N GPUs need an exchange that either loses samples' worth
// (averaging) or overshoots (summing stale deltas).  Here no
// row is ever replicated while it trains: GPU r owns the W rows of part r
// (equal source mass), the C table is cut into nb = 2N blocks (equal negative
// mass), and sub-round s trains cell (r, b = (2r + s) mod nb) on every GPU at
// once -- disjoint W rows, disjoint C rows.  After a sub-round GPU r passes
// block b to GPU r - 1, which trains it two sub-rounds later, so the transfer
// has a whole sub-round to overlap (group_blocks.cpp group_rotate, dist.py
// BlockSync).  The samples of a cell follow the one-GPU law restricted to the
// cell (train_blocks.hip); a call's samples are spread over the cells in
// proportion to their mass, so an epoch (nb sub-rounds) draws the one-GPU
// law of (source, context).  What changes is the order (cell by cell) and the
// negatives: drawn in the context's block (the law restricted to the block;
// blocks have equal negative mass), while a cell's sample count follows the
// block's CONTEXT mass -- so each cell weights its negative steps by the
// block's negative share over its sample share (cell_args, neg_law_on), and
// an epoch's expected negative updates per row are NegativeSample's.
#include <cmath>

#include "block_plan.h"
#include "train_host.h"

using namespace smore_host;

namespace {

constexpr uint64_t WALK_ROUND_MAX = (uint64_t)1 << 20;   // walks per prepared block round

int check_ctx(smore_ctx* c) {
    if (!c) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (c->device < 0) return fail(c, SMORE_ESTATE, "host-only context");
    return SMORE_OK;
}

BlockArgs block_args(const smore_ctx* c) {
    BlockArgs b{};
    b.atoms = c->blk.d_atoms;
    b.ntab = c->blk.d_ntab;
    b.nb = c->blk.nb;
    for (int k = 0; k <= c->blk.nb; ++k) b.cb[k] = (int32_t)c->blk.cb[k];
    b.hub_ntab = c->blk.d_hub_ntab;
    b.hub_off = c->blk.hub_off;
    b.nhub = (uint32_t)c->blk.nhub;
    b.H = (int32_t)c->blk.H;
    b.V = (int32_t)c->g->V;
    b.hub_of = c->blk.d_hub_of;
    return b;
}

// a probability as a Philox-word threshold (word < thr with probability p)
uint32_t prob_thr(double p) {
    const double t = std::ceil(std::ldexp(p, 32));
    return !(t > 0) ? 0u : t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
}

// the resident sample groups of this context's update launches (the hot
// tags' M): the same grid the training calls use
int64_t resident_groups(smore_ctx* c, bool walk, int K, int mode) {
    EdgeArgs a = record_args(c, SMORE_LINE2, K, mode);
    a.count = (uint64_t)1 << 30;
    a.alpha_rec = walk ? 1 : 0;
    a.sh_rows = mode == SMORE_HYBRID ? std::min(c->sh_max, sh_rows_max(c->dpad)) : 0;
    return (int64_t)edge_grid(c, UpdateFamily::Cpp, a) * (256 / lanes_of(c->dpad));
}

// per-block write-combined rows: the hottest hot C rows of each block under
// its cell's C-row law (pcb, flags hcb; entry i of block k is row cb[k] + i,
// or hub slot V + i - rows past the block's rows), with the edge rule's
// staleness bound and a two-tier drain (hot_maps.cpp build_hot_maps)
// Walk cells add their part's hottest W rows (key v | SH_WKEY, rate ps(v) N
// per record: wcand): the pair kernel keeps a run's W row in registers and
// flushed it atomically at the run's end, so C5's hub centre -- ~1 record
// runs, 16 % of its part's records at 8 parts -- queued every group's flush
// on one 512-B row (its part's cells 1.4x slower than the others'); combined,
// the block adds its groups' deltas in LDS and drains them on the row's
// interval (SMORE_WALK_WCOMB=1; off by default)
void block_sh_sets(smore_ctx* c, bool walk, bool on, int64_t Mg, const std::vector<std::vector<double>>& pcb,
                   const std::vector<std::vector<uint8_t>>& hcb, std::vector<int2>& hash, std::vector<int32_t>& ids,
                   const std::vector<std::pair<double, int32_t>>& wcand) {
    const int64_t V = c->g->V;
    auto& B = c->blk;
    const int cap = on ? std::max(0, std::min(c->sh_max, sh_rows_max(c->dpad))) : 0;
    B.sh_cap = std::max(cap, 1);
    B.sh_n.assign((size_t)B.nb, 0);
    B.sh_wn.assign((size_t)B.nb, 0);
    B.sh_lvl.assign((size_t)B.nb, std::array<int, 8>{});
    hash.assign((size_t)B.nb * SH_HASH, make_int2(-1, -1));
    ids.assign((size_t)B.nb * B.sh_cap, -1);
    const int flush_cap = c->sh_flush > 0 ? c->sh_flush : (walk ? PAIR_FLUSH_MAX : EDGE_FLUSH_MAX);
    B.sh_flush = flush_cap;
    if (cap == 0) return;
    const double M = (double)Mg, stale = sh_stale(walk), budget = cell_budget(walk);
    const bool two_tier = c->sh_flush <= 0;
    for (int k = 0; k < B.nb; ++k) {
        // A cell concentrates its samples on 1/nb of the C rows, so a hub row
        // takes about nb times its one-GPU share of a launch's updates (C4,
        // 8 GPUs: the top row ~18 % of a cell's C touches).  Each combined row
        // gets its own drain interval from its rate (power-of-two levels:
        // every slot every flush_cap rounds, each faster level's prefix at
        // its own interval), so the hubs stay within the staleness bound
        // without draining every other row as often.
        std::vector<std::pair<double, int32_t>> r;
        const int64_t rows = B.cb[k + 1] - B.cb[k];
        for (size_t i = 0; i < pcb[k].size(); ++i) {
            if (!hcb[k][i]) continue;
            const double p = pcb[k][i];
            const double f = two_tier ? (double)slot_interval(M * p, flush_cap, budget) : (double)flush_cap;
            const int64_t id = (int64_t)i < rows ? B.cb[k] + (int64_t)i : V + ((int64_t)i - rows);
            if (M * p * f <= stale) r.push_back({p, (int32_t)id});
        }
        for (const auto& x : wcand) {
            const double f = two_tier ? (double)slot_interval(M * x.first, flush_cap, budget) : (double)flush_cap;
            if (M * x.first * f <= stale) r.push_back(x);
        }
        const int64_t n = std::min<int64_t>(cap, (int64_t)r.size());
        std::partial_sort(r.begin(), r.begin() + n, r.end(), [](const auto& x, const auto& y) {
            return x.first > y.first || (x.first == y.first && x.second < y.second);
        });
        int2* h = hash.data() + (size_t)k * SH_HASH;
        for (int64_t i = 0; i < n; ++i) {
            B.sh_wn[k] += (r[i].second & SH_WKEY) ? 1 : 0;
            ids[(size_t)k * B.sh_cap + i] = r[i].second;
            uint32_t p = sh_hash_of(r[i].second);
            while (h[p & (SH_HASH - 1)].x >= 0) ++p;
            h[p & (SH_HASH - 1)] = make_int2(r[i].second, (int)i);
        }
        B.sh_n[k] = (int)n;
        if (two_tier && n > 0) {
            int lv[8];
            sh_levels(Mg, flush_cap, budget, r.data(), n, lv);
            std::copy(lv, lv + 8, B.sh_lvl[k].begin());
        }
        if (getenv("SMORE_SH_DEBUG")) {
            const auto& l = B.sh_lvl[k];
            fprintf(stderr, "[sh] block %d/%d M %lld rows %lld of %zu flush %d lvl %d %d %d %d %d %d %d %d top", k, B.nb,
                    (long long)Mg, (long long)n, r.size(), flush_cap, l[0], l[1], l[2], l[3], l[4], l[5], l[6], l[7]);
            for (int64_t i = 0; i < std::min<int64_t>(n, 4); ++i) fprintf(stderr, " %d:%.3g", r[i].second, M * r[i].first);
            fprintf(stderr, "\n");
        }
    }
}

// NegativeSample's law over an epoch (SMORE_NEG_LAW=0: off).  A cell (r, b)
// draws its K negatives from block b's restricted law, but the cells of part r
// get its samples in proportion to their CONTEXT mass m(r, b), while
// NegativeSample (src/proNet.cpp:623-633) would put a share pn(b) (~1/nb:
// blocks are cut to equal negative mass) of them in block b.  Scaling the
// cell's negative steps by pn(b) / m(r, b) makes part r's expected negative
// updates per row exactly the one-GPU ones (tests/test_blocks_cpu.py computes
// the epoch marginal).  LINE-2 cells take m(r, b) from the atoms' mass; walk
// cells from the round's record counts, on the device (neg_scale_of).
bool wcomb_on() {
    const char* e = getenv("SMORE_WALK_WCOMB");
    return e && atoi(e) != 0;
}

bool neg_law_on() {
    const char* e = getenv("SMORE_NEG_LAW");
    return !e || atoi(e) != 0;
}

// hub C rows of a block setup (smore_block_set_hubs / $SMORE_HUBS; -1:
// automatic), at most the C table's slot rows and half the vertices
// Automatic: none at 2 parts (a cell's rows are only 4 times hotter than
// one GPU's, and the hub copies' exchange costs more than it saves: C4 at
// 2^34 samples 1.057 vs 1.008 times one GPU's held-out loss), else 4096 --
// C4 at 8 parts: the five hub cells (10-14 ms against 7.7) disappear.
constexpr int64_t HUB_AUTO = 4096;
// The walk models the same (C5 DeepWalk at 8 parts: the capped hub cells
// and the 29 % rotation stall disappear, 1.34 -> 2.32x predicted) with their
// own exchange rule (c0 64, hub_c0: 1.026 times one GPU's held-out loss; c0
// 2048: 1.11).
int64_t hub_count(const smore_ctx* c, int64_t V, int nb) {
    int64_t h = c->blk_hubs;
    if (const char* e = getenv("SMORE_HUBS")) h = atoll(e);
    if (h < 0) h = nb <= 4 ? 0 : std::min<int64_t>(HUB_AUTO, V / (8 * (int64_t)nb));
    return std::max<int64_t>(0, std::min(std::min(h, c->c_slots), V / 2));
}

// walk cells' write-combined W candidates: the part's rows [wlo, whi) that
// are hot under the scaled source law
std::vector<std::pair<double, int32_t>> hot_w_rows(const std::vector<double>& ps, int64_t wlo, int64_t whi, int nparts,
                                                   int K, int64_t M, double tau) {
    std::vector<std::pair<double, int32_t>> wcand;
    // a W row's rate counts each record's 1 + K gradient terms against the
    // pair budget (SMORE_WALK_WCOMB_X overrides the factor)
    const char* xe = getenv("SMORE_WALK_WCOMB_X");
    const double wx = xe ? atof(xe) : (double)(1 + K);
    for (int64_t v = wlo; v < whi; ++v) {
        const double p = ps[v] * nparts * wx;
        if ((double)M * p > tau) wcand.push_back({p, (int32_t)(v | SH_WKEY)});
    }
    return wcand;
}

// the plan's host vectors, moved into the context
void keep_plan(smore_ctx::Blocks& B, BlockPlan& P) {
    B.wb = std::move(P.wb);
    B.cb = std::move(P.cb);
    B.mass = std::move(P.mass);
    B.part_mass = std::move(P.part_mass);
    B.nmass = std::move(P.nmass);
    B.atom_off = std::move(P.atom_off);
    B.hubs = std::move(P.hubs);
    B.hub_rate = std::move(P.hub_rate);
    B.hub_off = P.hub_off;
    B.nhub = P.nhub;
    B.hub_p = std::move(P.hub_p);
    B.pmax_w = std::move(P.pmax_w);
    B.pmax_c = std::move(P.pmax_c);
}

// the update-kernel arguments shared by a context's cell launches
EdgeArgs cell_args(smore_ctx* c, int k, bool walk) {
    const auto& B = c->blk;
    EdgeArgs a = record_args(c, SMORE_LINE2, B.K, B.mode);
    a.alpha_rec = walk ? 1 : 0;
    const bool on = B.mode == SMORE_HYBRID && B.sh_n[k] > 0;
    a.sh_rows = on ? B.sh_n[k] : 0;
    a.sh_hash = B.d_sh_hash + (size_t)k * SH_HASH;
    a.sh_ids = B.d_sh_ids + (size_t)k * B.sh_cap;
    a.sh_flush = std::max(1, B.sh_flush);
    a.sh_flush_w = 0;
    std::copy(B.sh_lvl[k].begin(), B.sh_lvl[k].end(), a.sh_lvl);
    // walk cells: cold W rows stored, not added (SMORE_WALK_WPLAIN=1; off:
    // measured no faster at C5, 8 parts -- 30.4 vs 31.6 ms per part's epoch)
    if (walk) {
        const char* e = getenv("SMORE_WALK_WPLAIN");
        a.w_plain = e && atoi(e) != 0;
        const char* x = getenv("SMORE_WALK_EDGE");   // walk cells through the edge kernel (study)
        a.rec_edge = x && atoi(x) != 0;
        a.w_comb = on && (size_t)k < B.sh_wn.size() && B.sh_wn[k] > 0;
    }
    if (neg_law_on() && (size_t)k < B.nmass.size()) {
        if (walk) {
            a.neg_scale = (float)B.nmass[k];
            a.neg_lo = B.d_off;
            a.neg_hi = B.d_off + (size_t)B.nb * B.walks;
        } else if ((size_t)k < B.mass.size() && B.mass[k] > 0) {
            a.neg_scale = (float)(B.nmass[k] / B.mass[k]);
        }
    }
    return a;
}

// A cell's launch: the context's grid, capped so that its hottest row takes
// at most SMORE_CELL_RATE concurrent updates per round (M p_max).  A cell
// concentrates its samples on 1/N of the W rows and 1/2N of the C rows, so
// its hub rows are up to 2N times as contended as at one GPU, where M p_max
// is ~130-260 (C5 DeepWalk, C2 LINE-2); Hogwild on a row with ~2000 updates in
// flight (C5 DeepWalk, 8 GPUs) diverges whether the row is atomic or
// write-combined.
int cell_grid(smore_ctx* c, const EdgeArgs& a, int k) {
    int grid = edge_grid(c, UpdateFamily::Cpp, a);
    const auto& B = c->blk;
    if (a.mode == SMORE_SERIAL || (size_t)k >= B.pmax_c.size()) return grid;
    // LINE-2 cells: the one-GPU launch's Hogwild concurrency cap (train.cpp
    // edge_grid: at most V / 16 resident sample groups) applied to the rows a
    // cell updates -- its block's C rows and the hub slots -- so a small
    // graph's cells (C2 at 8 GPUs: 62k rows per block) keep the one-GPU ratio
    // of in-flight updates per row instead of 16 times it
    if (a.alpha_rec == 0 && !getenv("SMORE_CELL_NOCAP")) {
        const int64_t rows = B.cb[k + 1] - B.cb[k] + B.H;
        const int gpb = 256 / lanes_of(c->dpad);
        const int64_t cap = std::max<int64_t>(8, (rows / 16 + gpb - 1) / gpb);
        if (cap < grid) grid = (int)cap;
    }
    double cap = a.alpha_rec == 1 ? CELL_RATE_PAIRS : CELL_RATE_EDGES;
    if (const char* e = getenv("SMORE_CELL_RATE")) cap = atof(e);
    // which side's hub sets the cap: both (default), SMORE_CELL_SIDE=c or w
    const char* side = getenv("SMORE_CELL_SIDE");
    const double pmax = side && side[0] == 'c' ? B.pmax_c[k]
                        : side && side[0] == 'w' ? B.pmax_w[k] : std::max(B.pmax_w[k], B.pmax_c[k]);
    if (cap <= 0 || pmax <= 0) return grid;
    const int gpb = 256 / lanes_of(c->dpad);
    const double groups = cap / pmax;
    const int g = std::max(8, (int)(groups / gpb) / 8 * 8);   // whole rounds of the 8 XCDs
    return std::min(grid, g);
}

}  // namespace

namespace smore_host {
// the exchange of the hub slots after every sub-round, one late (the rule of
// replica_sync.hip): slot j's summed delta is scaled by
// s + (1 - s) / N with s = min(1, c0 / k_j), k_j = its expected updates per
// exchange over all parts -- the sum for slots updated a few times per
// sub-round, towards the mean for the hubs that take hundreds of thousands
// (each part's copy reaches the same local equilibrium; summing N of them
// would overshoot)
void hub_scales(const smore_ctx::Blocks& B, double samples, double c0, float* out) {
    const double N = (double)B.n;
    for (int64_t j = 0; j < B.H; ++j) {
        const double k = B.hub_rate[j] * samples * N;
        const double s = k > 0 ? std::min(1.0, c0 / k) : 1.0;
        out[j] = (float)(s + (1.0 - s) / N);
    }
}

// launches per cell: with hub slots, 4 -- the slots are exchanged
// after each, so their copies are at most a quarter cell apart (C4, 8 parts:
// 1.042 times one GPU's held-out loss against 1.079 with one launch per
// cell, at 6.27 against 6.55 predicted); without, 1.  SMORE_CELL_LAUNCHES
// overrides (1..64).
int cell_launches(const smore_ctx::Blocks& B) {
    int k = B.H > 0 ? 4 : 1;
    if (const char* e = getenv("SMORE_CELL_LAUNCHES")) k = atoi(e);
    return std::max(1, std::min(64, k));
}

// largest remainder of n * mass[k] (ties to the lower index)
void largest_remainder(uint64_t n, const double* mass, int parts, uint64_t* counts) {
    std::vector<std::pair<double, int>> rem;
    uint64_t used = 0;
    for (int k = 0; k < parts; ++k) {
        const double x = (double)n * mass[k];
        counts[k] = (uint64_t)std::floor(x);
        used += counts[k];
        rem.push_back({x - std::floor(x), k});
    }
    std::stable_sort(rem.begin(), rem.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
    for (size_t i = 0; used < n && i < rem.size(); ++i, ++used) counts[rem[i].second]++;
    for (int k = 0; used < n; k = (k + 1) % parts, ++used) counts[k]++;   // rounding slack (never in practice)
}

int block_walks_gen(smore_ctx* c, int rule, uint64_t walk_begin, uint64_t walk_end, uint64_t gen_lo, uint64_t gen_hi,
                    int walk_times, int walk_steps, int window, int window_min, int K, double alpha0, uint64_t seed,
                    const int64_t* order, uint64_t order_base, int mode) {
    int rc;
    if ((rc = check_ctx(c))) return rc;
    auto& B = c->blk;
    if (!B.nb || B.model != SMORE_CENSUS) return fail(c, SMORE_ESTATE, "no walk block setup (smore_block_setup)");
    if (K != B.K || mode != B.mode) return fail(c, SMORE_EINVAL, "K / mode differ from smore_block_setup's");
    if (rule != 0 && rule != 1) return fail(c, SMORE_EINVAL, "block rounds: DeepWalk (0) or Walklets (1)");
    if ((rule == 0 && !order) || walk_times <= 0 || walk_steps < 0 || window <= 0)
        return fail(c, SMORE_EINVAL, "bad walk arguments");
    if (rule == 1 && (window_min < 0 || window_min > window)) return fail(c, SMORE_EINVAL, "Walklets: bad window");
    const uint64_t total = (uint64_t)walk_times * (uint64_t)c->g->V;
    if (walk_end > total) walk_end = total;
    B.walks = 0;
    if (walk_begin >= walk_end) return SMORE_OK;
    const uint64_t nw = walk_end - walk_begin;
    if (nw > WALK_ROUND_MAX) return fail(c, SMORE_EINVAL, "a block round holds at most 2^20 walks");
    if (gen_lo < walk_begin || gen_hi > walk_end || gen_lo > gen_hi)
        return fail(c, SMORE_EINVAL, "walk generation range outside the round");
    if (order) {
        if (walk_begin < order_base) return fail(c, SMORE_EINVAL, "walk order slice does not cover the range");
        order -= order_base;
        for (uint64_t i = walk_begin; i < walk_end; ++i)
            if (order[i] < 0 || order[i] >= c->g->V) return fail(c, SMORE_EINVAL, "walk start out of range");
    }
    if ((rc = set_device(c))) return rc;
    // the walk ids' tags: the scaled hot maps (a no-op when current)
    if (mode == SMORE_HYBRID) {
        const int64_t M = resident_groups(c, true, K, mode);
        if ((rc = build_hot_maps(c, SMORE_LINE2, K, M, HOT_TAU_WALK, PAIR_FLUSH_MAX, (double)B.n, (double)B.nb))) return rc;
    }
    if (order) {
        if ((rc = ensure_cap(c, c->d_order, c->order_cap, (size_t)nw))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->d_order, order + walk_begin, nw * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    }
    const int RW = rec_width(kmax_of(K));
    const uint64_t pb = std::max<uint64_t>(1, pair_bound(walk_steps, window, rule, window_min));
    if ((rc = ensure_cap(c, c->d_walks, c->walk_buf_n, (size_t)nw * (size_t)(walk_steps + 1)))) return rc;
    if ((rc = ensure_cap(c, c->d_lens, c->walk_lens_n, (size_t)nw))) return rc;
    const size_t ncount = (size_t)B.nb * nw + 1;
    if (B.count_cap < ncount) {
        dfree(B.d_count);
        dfree(B.d_off);
        B.count_cap = 0;
        HIPCHK(c, hipMalloc((void**)&B.d_count, ncount * sizeof(uint32_t)));
        HIPCHK(c, hipMalloc((void**)&B.d_off, ncount * sizeof(uint64_t)));
        B.count_cap = ncount;
    }
    if ((rc = ensure_cap(c, c->d_rec, c->rec_cap, (size_t)(nw * pb * RW)))) return rc;
    WalkArgs w;
    w.order = order ? c->d_order : nullptr;
    w.order_base = walk_begin;
    w.walks = c->d_walks;
    w.lens = c->d_lens;
    w.walk_begin = walk_begin;
    w.nwalks = nw;
    w.total_walks = total;
    w.steps = walk_steps;
    w.window = window;
    w.rule = rule;
    w.window_min = window_min;
    w.inv_p = w.inv_q = 1.0;
    w.wts = nullptr;
    w.nbr_sorted = nullptr;
    w.ntype = nullptr;
    w.ttargets = nullptr;
    w.toff = nullptr;
    w.paths = nullptr;
    w.path_off = nullptr;
    w.ntypes = w.npaths = 0;
    w.slot_extra = 0;
    w.own_lo = (int32_t)B.wb[B.r];
    w.own_hi = (int32_t)B.wb[B.r + 1];
    B.wargs = w;
    B.wseed = seed;
    B.walpha0 = alpha0;
    B.wpairs = pb;
    B.walks = nw;
    B.rec_bound = nw * pb;
    if (gen_hi > gen_lo) {   // this context's share of the round's walks
        WalkArgs wg = w;
        const uint64_t o = gen_lo - walk_begin;
        wg.walk_begin = gen_lo;
        wg.nwalks = gen_hi - gen_lo;
        wg.walks = w.walks + o * (uint64_t)(walk_steps + 1);
        wg.lens = w.lens + o;
        HIPCHK(c, launch_walk_gen(dev_graph(c), wg, seed, c->stream));
    }
    return SMORE_OK;
}

int block_walks_emit(smore_ctx* c) {
    auto& B = c->blk;
    if (!B.walks) return SMORE_OK;
    const WalkArgs& w = B.wargs;
    const size_t ncount = (size_t)B.nb * B.walks + 1;
    const BlockArgs ba = block_args(c);
    HIPCHK(c, hipMemsetAsync(B.d_count + (ncount - 1), 0, sizeof(uint32_t), c->stream));
    HIPCHK(c, launch_block_pair_count(w, ba, B.wseed, B.d_count, c->stream));
    HIPCHK(c, scan_pair_counts(B.d_count, B.d_off, ncount, &c->d_scan_tmp, &c->scan_tmp_bytes, c->stream));
    HIPCHK(c, launch_block_pair_emit(w, ba, B.wseed, B.K, B.walpha0, B.d_off, c->d_rec, c->stream));
    return SMORE_OK;
}


void blocks_release(smore_ctx* c) {
    auto& B = c->blk;
    dfree(B.d_atoms);
    dfree(B.d_ntab);
    dfree(B.d_sh_hash);
    dfree(B.d_sh_ids);
    dfree(B.d_count);
    dfree(B.d_off);
    dfree(B.d_hub_ntab);
    dfree(B.d_hub_ids);
    dfree(B.d_hub_of);
    for (float*& p : B.d_hub_ex) dfree(p);
    dfree(B.d_hub_scale);
    B = smore_ctx::Blocks{};
}
}  // namespace smore_host

extern "C" {

int smore_block_setup(smore_ctx* c, int model, int nparts, int part, int K, int mode) {
    int rc;
    if ((rc = check_ctx(c))) return rc;
    if (model != SMORE_LINE2 && model != SMORE_CENSUS)
        return fail(c, SMORE_EINVAL, "block schedule: LINE-2 (SMORE_LINE2) or the C++ walk models (SMORE_CENSUS)");
    if (nparts < 1 || 2 * nparts > BLOCK_MAX || part < 0 || part >= nparts)
        return fail(c, SMORE_EINVAL, "block schedule: 1 <= nparts <= 16, 0 <= part < nparts");
    if (K < 0 || K > (model == SMORE_LINE2 ? 20 : 10) || mode < 0 || mode > 3)
        return fail(c, SMORE_EINVAL, "block schedule: bad K / mode");
    if (c->semantics != SMORE_SEM_CPP) return fail(c, SMORE_EINVAL, "block schedule: C++ rules only");
    if (c->ntables < 2) return fail(c, SMORE_ESTATE, "block schedule: W and C tables needed");
    if (int rc_ = refuse_cse(c)) return rc_;
    if ((rc = set_device(c))) return rc;
    const bool walk = model == SMORE_CENSUS;
    if (nparts == 1) {
        blocks_release(c);
        return SMORE_OK;
    }
    const HostGraph& g = *c->g;
    const int64_t V = g.V;
    const int nb = 2 * nparts;
    if (V < nb) return fail(c, SMORE_EINVAL, "block schedule: fewer vertices than blocks");
    const int64_t H = hub_count(c, V, nb);
    char key[288];
    snprintf(key, sizeof key, "%d/%d/%d/%d/%d/%lld/%lld/%d/%d/%d/%.9g/%lld/%s", model, nparts, part, K, mode,
             (long long)V, (long long)g.E, c->dpad, c->sh_max, c->sh_flush, c->hot_tau, (long long)H,
             getenv("SMORE_SH_STALE") ? getenv("SMORE_SH_STALE") : "");
    if (c->blk.key == key) return SMORE_OK;
    blocks_release(c);
    auto& B = c->blk;
    // Hot tags (hybrid scatter) and the write-combined sets.  LINE-2: exact
    // per cell from its atoms (block_plan.cpp line2_cell_law).  Walks: the
    // scaled global law (hot_maps.cpp build_hot_maps), whose tags the walk
    // ids carry.
    const bool hyb = mode == SMORE_HYBRID;
    int64_t M = 0;
    double tau = 0.0;
    bool small = false;
    if (hyb) {
        M = resident_groups(c, walk, K, mode);
        small = c->hot_tau < 0 && 16.0 * (double)M >= (double)V;
        // LINE-2 cells at 3-4 parts of a large graph: tau 0.6 (their rows are
        // 6-8x hotter than one GPU's, not 16x: C4 at 4 parts 1.037-1.040x one
        // GPU's held-out loss at 3.60x predicted, against 1.034x at 3.39x with
        // 0.3; at 8 parts 0.6 costs 1.054x; C2 -- 1M vertices, 125k rows per
        // block at 4 parts -- 1.048x, so graphs under 4M vertices keep 0.3;
        // DESIGN.md 10.6)
        const bool t06 = !walk && nparts >= 3 && nparts <= 4 && V >= ((int64_t)1 << 22);
        const double tcell = t06 ? 0.6 : (walk ? HOT_TAU_WALK : HOT_TAU_CELL);
        tau = c->hot_tau >= 0 ? c->hot_tau : small ? 0.0 : tcell;
        if (walk && (rc = build_hot_maps(c, SMORE_LINE2, K, M, HOT_TAU_WALK, PAIR_FLUSH_MAX, (double)nparts, (double)nb))) return rc;
    }
    DrawLaws laws;
    draw_probabilities(g, laws.ps, laws.pn, laws.pc);
    const BlockPlanArgs pa{walk, nparts, part, K, hyb, H, M, tau, walk && hyb ? c->hot_c.data() : nullptr};
    BlockPlan P;
    const std::string why = build_block_plan(g, laws, pa, P);
    if (!why.empty()) return fail(c, SMORE_EINVAL, why);
    B.n = nparts;
    B.r = part;
    B.nb = nb;
    B.model = model;
    B.K = K;
    B.mode = mode;
    B.H = H;
    keep_plan(B, P);
    c->hot_M = M;
    std::vector<int2> hash;
    std::vector<int32_t> ids;
    // walk cells: the part's hot W rows (block_sh_sets)
    std::vector<std::pair<double, int32_t>> wcand;
    if (walk && hyb && wcomb_on()) wcand = hot_w_rows(laws.ps, B.wb[part], B.wb[part + 1], nparts, K, M, tau);
    block_sh_sets(c, walk, hyb && !small, M, P.pcb, P.hcb, hash, ids, wcand);
    if (getenv("SMORE_SH_DEBUG"))
        for (int k = 0; k < nb; ++k)
            fprintf(stderr, "[cell] part %d/%d block %d M %lld M*pmax_w %.4g M*pmax_c %.4g hubs %lld hub_p %.4g\n", part,
                    nparts, k, (long long)M, M * B.pmax_w[k], M * B.pmax_c[k], (long long)H, B.hub_p[k]);
    if ((rc = upload(c, B.d_ntab, reinterpret_cast<const uint2*>(P.ntab.data()), (size_t)V, true))) return rc;
    if (H > 0) {
        if ((rc = upload(c, B.d_hub_ntab, reinterpret_cast<const uint2*>(P.hub_ntab.data()), P.hub_ntab.size()))) return rc;
        if ((rc = upload(c, B.d_hub_ids, B.hubs.data(), B.hubs.size()))) return rc;
        if (walk && (rc = upload(c, B.d_hub_of, P.hub_of.data(), P.hub_of.size()))) return rc;
    }
    if (!walk && (rc = upload(c, B.d_atoms, reinterpret_cast<const uint4*>(P.atoms.data()), P.atoms.size() / 4, true)))
        return rc;
    if ((rc = upload(c, B.d_sh_hash, hash.data(), hash.size()))) return rc;
    if ((rc = upload(c, B.d_sh_ids, ids.data(), ids.size()))) return rc;
    B.key = key;
    return SMORE_OK;
}

int smore_block_set_hubs(smore_ctx* c, int64_t hubs) {
    if (!c || hubs < -1) return SMORE_EINVAL;
    c->blk_hubs = hubs;
    return SMORE_OK;
}

int smore_block_hubs(const smore_ctx* c, int64_t* H, int64_t* first_slot, int32_t* rows, double* rates) {
    if (!c) return SMORE_EINVAL;
    if (!c->blk.nb) return SMORE_ESTATE;
    const auto& B = c->blk;
    if (H) *H = B.H;
    if (first_slot) *first_slot = c->g->V;
    if (rows) std::copy(B.hubs.begin(), B.hubs.end(), rows);
    if (rates) std::copy(B.hub_rate.begin(), B.hub_rate.end(), rates);
    return SMORE_OK;
}

int smore_block_hubs_load(smore_ctx* c) {
    int rc;
    if ((rc = check_ctx(c))) return rc;
    if (!c->blk.nb) return fail(c, SMORE_ESTATE, "no block setup");
    if (!c->blk.H) return SMORE_OK;
    if ((rc = set_device(c))) return rc;
    float* C = c->d_table[1];
    HIPCHK(c, launch_rows_gather(C, c->blk.d_hub_ids, (uint64_t)c->blk.H, c->dpad, C + (size_t)c->g->V * c->dpad,
                                 c->stream));
    return SMORE_OK;
}

int smore_block_hubs_store(smore_ctx* c) {
    int rc;
    if ((rc = check_ctx(c))) return rc;
    if (!c->blk.nb) return fail(c, SMORE_ESTATE, "no block setup");
    if (!c->blk.H) return SMORE_OK;
    if ((rc = set_device(c))) return rc;
    float* C = c->d_table[1];
    HIPCHK(c, launch_rows_scatter(C, c->blk.d_hub_ids, (uint64_t)c->blk.H, c->dpad, C + (size_t)c->g->V * c->dpad,
                                  c->stream));
    return SMORE_OK;
}

int smore_block_cell_launches(const smore_ctx* c) {
    if (!c || !c->blk.nb) return 1;
    return cell_launches(c->blk);
}

int smore_block_hub_scales(const smore_ctx* c, double samples, double c0, float* scales) {
    if (!c || !scales || !(samples > 0.0) || !(c0 > 0.0)) return SMORE_EINVAL;
    if (!c->blk.nb) return SMORE_ESTATE;
    hub_scales(c->blk, samples, c0, scales);
    return SMORE_OK;
}

int smore_block_info(const smore_ctx* c, int* nparts, int* part, int* nblocks) {
    if (!c) return SMORE_EINVAL;
    if (nparts) *nparts = c->blk.nb ? c->blk.n : 1;
    if (part) *part = c->blk.nb ? c->blk.r : 0;
    if (nblocks) *nblocks = c->blk.nb;
    return SMORE_OK;
}

int smore_block_bounds(const smore_ctx* c, int64_t* wb, int64_t* cb) {
    if (!c) return SMORE_EINVAL;
    if (!c->blk.nb) return SMORE_ESTATE;
    if (wb) std::copy(c->blk.wb.begin(), c->blk.wb.end(), wb);
    if (cb) std::copy(c->blk.cb.begin(), c->blk.cb.end(), cb);
    return SMORE_OK;
}

int smore_block_mass(const smore_ctx* c, double* mass) {
    if (!c || !mass) return SMORE_EINVAL;
    if (!c->blk.nb || c->blk.model != SMORE_LINE2) return SMORE_ESTATE;
    std::copy(c->blk.mass.begin(), c->blk.mass.end(), mass);
    return SMORE_OK;
}

int smore_block_part_mass(const smore_ctx* c, double* mass) {
    if (!c || !mass) return SMORE_EINVAL;
    if (!c->blk.nb || c->blk.model != SMORE_LINE2) return SMORE_ESTATE;
    std::copy(c->blk.part_mass.begin(), c->blk.part_mass.end(), mass);
    return SMORE_OK;
}

int smore_block_neg_scale(const smore_ctx* c, int block, double* w) {
    if (!c || !w) return SMORE_EINVAL;
    if (!c->blk.nb || c->blk.model != SMORE_LINE2) return SMORE_ESTATE;
    if (block < 0 || block >= c->blk.nb) return SMORE_EINVAL;
    const EdgeArgs a = cell_args(const_cast<smore_ctx*>(c), block, false);
    *w = a.neg_scale > 0.0f ? (double)a.neg_scale : 1.0;
    return SMORE_OK;
}

int smore_block_counts(const smore_ctx* c, uint64_t samples, uint64_t* counts) {
    if (!c || !counts) return SMORE_EINVAL;
    if (!c->blk.nb || c->blk.model != SMORE_LINE2) return SMORE_ESTATE;
    largest_remainder(samples, c->blk.mass.data(), c->blk.nb, counts);
    return SMORE_OK;
}

int smore_block_train_edges_async(smore_ctx* c, int block, uint64_t begin, uint64_t count, uint64_t total, int K,
                                  double alpha0, uint64_t seed, int mode) {
    int rc;
    if ((rc = check_ctx(c))) return rc;
    auto& B = c->blk;
    if (!B.nb || B.model != SMORE_LINE2) return fail(c, SMORE_ESTATE, "no LINE-2 block setup (smore_block_setup)");
    if (block < 0 || block >= B.nb) return fail(c, SMORE_EINVAL, "block out of range");
    if (K != B.K || mode != B.mode) return fail(c, SMORE_EINVAL, "K / mode differ from smore_block_setup's");
    if (total == 0) return fail(c, SMORE_EINVAL, "total == 0");
    if (count == 0) return SMORE_OK;
    if ((rc = set_device(c))) return rc;
    const uint64_t na = B.atom_off[block + 1] - B.atom_off[block];
    if (na == 0 && B.nhub == 0) return fail(c, SMORE_EINVAL, "block without atoms (mass 0) asked for samples");
    EdgeArgs a = cell_args(c, block, false);
    if (const char* e = getenv("SMORE_EDGE_CHUNK")) a.pair_slice = (uint32_t)std::max(0, atoi(e));
    a.total = total;
    a.seed = seed;
    a.alpha0 = alpha0;
    a.count = count;
    const int grid = cell_grid(c, a, block);
    BlockArgs ba = block_args(c);
    ba.atom_off = B.atom_off[block];
    ba.natoms = (uint32_t)na;
    ba.hub_thr = B.nhub ? prob_thr(B.hub_p[block]) : 0u;
    const int RW = rec_width(kmax_of(K));
    const uint64_t chunk_max = mode == SMORE_SERIAL ? ((uint64_t)1 << 30) / (uint64_t)RW : (uint64_t)1 << 27;
    const uint64_t chunk = std::min<uint64_t>(count, chunk_max);
    const int nch = (int)((count + chunk - 1) / chunk);
    if ((rc = ensure_cap(c, c->d_rec, c->rec_cap, (size_t)(chunk * RW)))) return rc;
    if ((rc = grow_events(c, c->phase_ev, 2 * (size_t)nch + 1))) return rc;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    HIPCHK(c, hipEventRecord(c->phase_ev[0], c->stream));
    for (int k = 0; k < nch; ++k) {
        const uint64_t b = (uint64_t)k * chunk, n = std::min<uint64_t>(chunk, count - b);
        if (k) HIPCHK(c, hipEventRecord(c->phase_ev[2 * k], c->stream));
        HIPCHK(c, launch_block_draw(ba, block, seed, begin + b, n, K, c->d_rec, c->stream));
        HIPCHK(c, hipEventRecord(c->phase_ev[2 * k + 1], c->stream));
        EdgeArgs ak = a;
        ak.begin = begin + b;
        ak.count = n;
        ak.rec = c->d_rec;
        HIPCHK(c, hipMemsetAsync(c->d_work, 0, sizeof(unsigned long long), c->stream));
        HIPCHK(c, launch_update(update_kernel(UpdateFamily::Cpp, ak), ak, grid, c->stream));
        HIPCHK(c, hipEventRecord(c->phase_ev[2 * k + 2], c->stream));
    }
    return finish_timed(c, mode, nch);
}

int smore_block_sample_edges(smore_ctx* c, int block, uint64_t seed, uint64_t begin, uint64_t count, int K,
                             int32_t* out) {
    int rc;
    if ((rc = check_ctx(c))) return rc;
    if (!out) return SMORE_EINVAL;
    auto& B = c->blk;
    if (!B.nb || B.model != SMORE_LINE2) return fail(c, SMORE_ESTATE, "no LINE-2 block setup (smore_block_setup)");
    if (block < 0 || block >= B.nb || K < 0 || K > 20) return fail(c, SMORE_EINVAL, "bad block / K");
    if (count == 0) return SMORE_OK;
    if ((rc = set_device(c))) return rc;
    BlockArgs ba = block_args(c);
    ba.atom_off = B.atom_off[block];
    ba.natoms = (uint32_t)(B.atom_off[block + 1] - B.atom_off[block]);
    ba.hub_thr = B.nhub ? prob_thr(B.hub_p[block]) : 0u;
    if (ba.natoms == 0 && B.nhub == 0) return fail(c, SMORE_EINVAL, "block without atoms");
    const int RW = rec_width(kmax_of(K));
    int32_t* d = nullptr;
    HIPCHK(c, hipMalloc((void**)&d, count * RW * sizeof(int32_t)));
    hipError_t e = launch_block_draw(ba, block, seed, begin, count, K, d, c->stream);
    std::vector<int32_t> h(count * RW);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(h.data(), d, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(c, SMORE_EHIP, std::string("block sample: ") + hipGetErrorString(e));
    for (uint64_t t = 0; t < count; ++t)
        for (int j = 0; j < 2 + K; ++j) out[t * (2 + K) + j] = h[t * RW + j] & ID_MASK;
    return SMORE_OK;
}

int smore_block_walks_generate(smore_ctx* c, int rule, uint64_t walk_begin, uint64_t walk_end, uint64_t gen_lo,
                               uint64_t gen_hi, int walk_times, int walk_steps, int window, int window_min, int K,
                               double alpha0, uint64_t seed, const int64_t* order, uint64_t order_base, int mode) {
    return block_walks_gen(c, rule, walk_begin, walk_end, gen_lo, gen_hi, walk_times, walk_steps, window, window_min,
                           K, alpha0, seed, order, order_base, mode);
}

int smore_block_walks_emit(smore_ctx* c) {
    int rc;
    if ((rc = check_ctx(c))) return rc;
    if ((rc = set_device(c))) return rc;
    return block_walks_emit(c);
}

int smore_block_walks_buffer(smore_ctx* c, void** walks, void** lens, int64_t* stride) {
    if (!c) return SMORE_EINVAL;
    if (walks) *walks = c->d_walks;
    if (lens) *lens = c->d_lens;
    if (stride) *stride = (int64_t)c->blk.wargs.steps + 1;
    return SMORE_OK;
}

int smore_block_prepare_walks(smore_ctx* c, int rule, uint64_t walk_begin, uint64_t walk_end, int walk_times,
                              int walk_steps, int window, int window_min, int K, double alpha0, uint64_t seed,
                              const int64_t* order, uint64_t order_base, int mode) {
    int rc = block_walks_gen(c, rule, walk_begin, walk_end, walk_begin, walk_end, walk_times, walk_steps, window,
                             window_min, K, alpha0, seed, order, order_base, mode);
    if (rc) return rc;
    return block_walks_emit(c);
}

int smore_block_train_walks_async(smore_ctx* c, int block) { return smore_block_train_walks_part_async(c, block, 0, 1); }

int smore_block_train_walks_part_async(smore_ctx* c, int block, int part, int parts) {
    int rc;
    if ((rc = check_ctx(c))) return rc;
    if (parts < 1 || part < 0 || part >= parts) return fail(c, SMORE_EINVAL, "bad bucket part");
    auto& B = c->blk;
    if (!B.nb || B.model != SMORE_CENSUS) return fail(c, SMORE_ESTATE, "no walk block setup (smore_block_setup)");
    if (block < 0 || block >= B.nb) return fail(c, SMORE_EINVAL, "block out of range");
    if (!B.walks) return SMORE_OK;   // an empty round
    if ((rc = set_device(c))) return rc;
    EdgeArgs a = cell_args(c, block, true);
    a.total = 1;
    a.rec = c->d_rec;
    a.count = B.rec_bound;   // the grid's bound; the launch reads its range on the device
    a.rec_base = B.d_off + (size_t)block * B.walks;
    a.count_dev = B.d_off + (size_t)(block + 1) * B.walks;
    a.part_q = (uint32_t)part;
    a.part_n = (uint32_t)parts;
    const int grid = B.mode == SMORE_SERIAL ? 1 : cell_grid(c, a, block);
    HIPCHK(c, hipMemsetAsync(c->d_work, 0, sizeof(unsigned long long), c->stream));
    HIPCHK(c, launch_update(update_kernel(UpdateFamily::Cpp, a), a, grid, c->stream));
    return SMORE_OK;
}

int smore_block_walk_records(smore_ctx* c, int block, uint64_t* n) {
    if (!c || !n) return SMORE_EINVAL;
    auto& B = c->blk;
    if (!B.nb || B.model != SMORE_CENSUS || block < 0 || block >= B.nb) return SMORE_EINVAL;
    *n = 0;
    if (!B.walks) return SMORE_OK;
    uint64_t lo = 0, hi = 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(&lo, B.d_off + (size_t)block * B.walks, sizeof lo, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&hi, B.d_off + (size_t)(block + 1) * B.walks, sizeof hi, hipMemcpyDeviceToHost));
    *n = hi - lo;
    return SMORE_OK;
}

int smore_block_walk_records_copy(smore_ctx* c, int block, int32_t* out, uint64_t cap, uint64_t* n, int* width) {
    if (!c || !n || !width) return SMORE_EINVAL;
    auto& B = c->blk;
    if (!B.nb || B.model != SMORE_CENSUS || block < 0 || block >= B.nb) return SMORE_EINVAL;
    const int RW = rec_width(kmax_of(B.K));
    *width = RW;
    *n = 0;
    if (!B.walks) return SMORE_OK;
    uint64_t lo = 0, hi = 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(&lo, B.d_off + (size_t)block * B.walks, sizeof lo, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&hi, B.d_off + (size_t)(block + 1) * B.walks, sizeof hi, hipMemcpyDeviceToHost));
    *n = hi - lo;
    if (!out) return SMORE_OK;
    if (cap < hi - lo) return fail(c, SMORE_EINVAL, "walk records: buffer too small");
    if (hi > lo)
        HIPCHK(c, hipMemcpy(out, static_cast<const int32_t*>(c->d_rec) + lo * RW, (hi - lo) * RW * sizeof(int32_t),
                            hipMemcpyDeviceToHost));
    return SMORE_OK;
}

}  // extern "C"

// train.cpp -- the training drivers of the C ABI: each turns a call into
// records on the device (drawn edges, walk pairs, APP / HPE records, caller
// pairs) and runs them through the update kernel of the scatter mode.  The
// launch plan and the per-chunk update launch are written once, here.
#include "train_host.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

using namespace smore_host;

namespace smore_host {

int edge_grid(smore_ctx* c, const UpdateKernel& k, int mode, uint64_t count, bool leave_slot) {
    if (mode == SMORE_SERIAL) return 1;
    int per_cu = 0;
    if (!k.fn || hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.fn, 256, k.lds) != hipSuccess || per_cu < 1)
        per_cu = 1;
    // leave one block slot per CU to the concurrent draw kernel (measured at C4:
    // 3 of 4 update blocks per CU run the update as fast as 4)
    if (leave_slot && per_cu > 1) per_cu -= 1;
    // tuning knob: SMORE_BLOCKS_PER_CU caps the resident blocks per CU
    if (const char* e = getenv("SMORE_BLOCKS_PER_CU")) {
        const int cap = atoi(e);
        if (cap > 0 && cap < per_cu) per_cu = cap;
    }
    int64_t grid = (int64_t)c->cus * per_cu;
    // tuning knob: SMORE_MAX_BLOCKS caps the whole grid
    if (const char* e = getenv("SMORE_MAX_BLOCKS")) {
        const int64_t cap = atoll(e);
        if (cap > 0 && cap < grid) grid = cap;
    }
    const int G = lanes_of(c->dpad);
    const int64_t groups_per_block = 256 / G;
    const int64_t need = ((int64_t)count + groups_per_block - 1) / groups_per_block;
    if (need < grid) grid = need;
    // Hogwild concurrency cap: at most V/16 resident sample groups (each keeps
    // two samples in flight), so that on small graphs the expected number of
    // in-flight updates per row stays O(1) as in the reference's few-thread
    // Hogwild; the benchmark graphs (V >= 1M) are far from the cap.
    const int64_t cap_groups = std::max<int64_t>(1, c->g->V / 16);
    const int64_t cap = (cap_groups + groups_per_block - 1) / groups_per_block;
    if (cap < grid) grid = cap;
    return (int)(grid < 1 ? 1 : grid);
}

int grow_events(smore_ctx* c, std::vector<hipEvent_t>& v, size_t n) {
    while (v.size() < n) {
        hipEvent_t e;
        HIPCHK(c, hipEventCreate(&e));
        v.push_back(e);
    }
    return SMORE_OK;
}

EdgeArgs record_args(smore_ctx* c, int model, int K, int mode) {
    EdgeArgs a{};
    a.g = dev_graph(c);
    a.sig = c->d_sig;
    a.W = c->d_table[0];
    a.C = model == SMORE_LINE2 ? c->d_table[1] : c->d_table[0];
    a.skipped = c->d_skipped;
    a.dpad = c->dpad;
    a.K = K;
    a.model = model;
    a.mode = mode;
    a.tcum = c->d_tcum;
    a.work = c->d_work;
    return a;
}

int plan_record_launch(smore_ctx* c, EdgeArgs& a, bool combine, UpdateFamily f, int hot_model, double tau_default,
                       int flush_max, int* grid) {
    a.sh_rows = combine ? std::min(c->sh_max, sh_rows_max(c->dpad)) : 0;   // LDS bound for the grid
    *grid = edge_grid(c, f, a);
    if (a.mode == SMORE_HYBRID) {
        const int64_t M = (int64_t)*grid * (256 / lanes_of(c->dpad));
        int rc;
        if ((rc = build_hot_maps(c, hot_model, a.K, M, tau_default, flush_max))) return rc;
    }
    a.sh_rows = combine ? c->sh_rows : 0;
    a.sh_hash = c->d_sh_hash;
    a.sh_ids = c->d_sh_ids;
    a.sh_flush = std::max(1, c->sh_flush_eff);
    a.sh_flush_w = c->sh_flush_w_eff;
    std::copy(std::begin(c->sh_lvl_eff), std::end(c->sh_lvl_eff), a.sh_lvl);
    return SMORE_OK;
}

int plan_pair_records(smore_ctx* c, UpdateFamily f, int K, int mode, uint64_t total, uint64_t seed, double alpha0,
                      double reg, uint64_t max_records, EdgeArgs* a, int* grid) {
    *a = record_args(c, SMORE_LINE2, K, mode);
    a->total = total;
    a->seed = seed;
    a->alpha0 = alpha0;
    a->reg = (float)reg;
    a->alpha_rec = 1;
    a->count = max_records;   // the grid for the most records a chunk can have
    int rc;
    if ((rc = plan_record_launch(c, *a, mode == SMORE_HYBRID, f, SMORE_LINE2, HOT_TAU_WALK, PAIR_FLUSH_MAX, grid)))
        return rc;
    a->g = dev_graph(c);   // the tables as the hot maps left them
    a->rec = c->d_rec;
    return SMORE_OK;
}

int launch_record_update(smore_ctx* c, UpdateFamily f, const EdgeArgs& ak, int grid) {
    HIPCHK(c, hipMemsetAsync(c->d_work, 0, sizeof(unsigned long long), c->stream));
    const int g = ak.mode == SMORE_SERIAL ? 1 : grid;
    if (c->census)
        HIPCHK(c, launch_row_census(ak.rec, ak.count, ak.count_dev, rec_width(kmax_of(ak.K)), ak.K, c->d_census[0],
                                    c->d_census[1], c->cus, c->stream));
    else HIPCHK(c, launch_update(update_kernel(f, ak), ak, g, c->stream));
    return SMORE_OK;
}

int finish_timed(smore_ctx* c, int mode, int phase_n) {
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->timed = true;
    c->last_mode = mode;
    c->phase_n = phase_n;
    return SMORE_OK;
}

int sync_after(smore_ctx* c, int rc, bool check_last_error) {
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (check_last_error) HIPCHK(c, hipGetLastError());
    return SMORE_OK;
}

}  // namespace smore_host

// the hot/cold record split of the C++ edge models' hybrid scatter (train_draw.hip
// draw_split_kernel): off unless SMORE_SPLIT is set to a non-zero number
static bool split_on() {
    static const int env = [] {
        const char* e = getenv("SMORE_SPLIT");
        return e ? atoi(e) : -1;
    }();
    return env > 0;
}

extern "C" {

int smore_train_edges_async(smore_ctx* c, int model, uint64_t begin, uint64_t count, uint64_t total, int K,
                            double alpha0, double reg, uint64_t seed, int mode) {
    if (!c) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (model < 0 || model > 3 || mode < 0 || mode > 3 || K < 0 || K > 20)
        return fail(c, SMORE_EINVAL, "bad model/mode/K");
    const int need_tables = model == SMORE_LINE2 ? 2 : 1;
    if (c->ntables < need_tables) return fail(c, SMORE_ESTATE, "tables not allocated");
    if (int rc_ = refuse_cse(c)) return rc_;
    if (total == 0) return fail(c, SMORE_EINVAL, "total == 0");
    if (c->census)
        return fail(c, SMORE_ESTATE, "row census: edge models have exact rates (smore_row_rates with their model)");
    if (count == 0) return SMORE_OK;
    int rc;
    if ((rc = set_device(c))) return rc;
    EdgeArgs a = record_args(c, model, model == SMORE_BPR ? 5 : K, mode);
    a.begin = begin;
    a.count = count;
    a.total = total;
    a.seed = seed;
    a.alpha0 = alpha0;
    a.reg = (float)reg;
    // Go semantics (SMORE_SEM_GO): Go draws into the same records
    // (go_draw_kernel) and the Go rules on them (go_rec.h), with every
    // scatter mode; BPR is Go's two-table, one-negative rule
    const bool go = c->semantics == SMORE_SEM_GO;
    const UpdateFamily fam = go ? UpdateFamily::GoRec : UpdateFamily::Cpp;
    if (go) {
        if (model == SMORE_MF) return fail(c, SMORE_EINVAL, "Go semantics has no MF model");
        if (K > 10) return fail(c, SMORE_EINVAL, "Go semantics: K <= 10");
        if (model == SMORE_BPR && c->ntables < 2) return fail(c, SMORE_ESTATE, "Go BPR needs W (users) and C (items)");
        if (model == SMORE_BPR) {
            a.C = c->d_table[1];
            a.K = 1;
        } else {
            a.K = K;
        }
    }
    // C++ BPR's hybrid runs the plain-store kernel on graphs above the
    // small-graph cap (16 M < V; below it every row is hot and the hybrid is
    // the atomic scatter): C3 at 2^28 samples, held-out BPR objective +0.11 %
    // of the atomic scatter's and the same ranking accuracy (0.82548 vs
    // 0.82549), update 80.3 ms per 2^26 against the tagged kernel's 97.6 -- its
    // ~170 hot rows are hub items drawn as positives, whose collisions cost
    // less than the hybrid kernel's code shape (2 blocks per CU against 3;
    // DESIGN.md 8, profiles/r05/bpr).  SMORE_BPR_SCATTER=tagged keeps the
    // tagged hybrid kernel.
    if (model == SMORE_BPR && !go && mode == SMORE_HYBRID) {
        const char* e = getenv("SMORE_BPR_SCATTER");
        EdgeArgs t = a;
        t.sh_rows = 0;
        const int64_t Mb = (int64_t)edge_grid(c, UpdateFamily::Cpp, t) * (256 / lanes_of(c->dpad));
        const bool small = c->hot_tau < 0 && 16.0 * (double)Mb >= (double)c->g->V;
        if (!small && !(e && !strcmp(e, "tagged"))) a.mode = mode = SMORE_HOGWILD;
    }
    // C++ BPR combines its hub rows only with SMORE_BPR_COMBINE=1 (measured in
    // the hub items are positives, the negatives are uniform)
    const char* bpr_comb = getenv("SMORE_BPR_COMBINE");
    const bool combine = mode == SMORE_HYBRID && (go || model != SMORE_BPR || (bpr_comb && atoi(bpr_comb) != 0));
    // Go BPR has two tables (users W, items C): the LINE-2 row roles
    const int hot_model = go && model == SMORE_BPR ? SMORE_LINE2 : model;
    int grid;
    if ((rc = plan_record_launch(c, a, combine, fam, hot_model, go ? HOT_TAU_WALK : HOT_TAU_EDGE,
                                 EDGE_FLUSH_MAX, &grid)))
        return rc;
    // edge models: draw kernel -> update kernel per chunk of samples.  With
    // several chunks the draws of chunk k+1 run on a second stream while
    // chunk k updates (two record buffers; the update kernel leaves one block
    // slot per CU for them).  Both kernels are bound by HBM, so the overlap
    // buys little (C4 hybrid, 2^25-sample chunks: 120.4 ms per 2^27 samples
    // vs 122 sequential; plain stores 116.6 vs 108): chunks default to 2^27
    // samples (SMORE_DRAW_CHUNK overrides), i.e. sequential for a bench step.
    const int RW = rec_width(kmax_of(a.K));
    uint64_t chunk_max = (uint64_t)1 << 27;
    if (const char* e = getenv("SMORE_DRAW_CHUNK")) chunk_max = std::max<uint64_t>(1024, strtoull(e, nullptr, 10));
    if (a.mode == SMORE_SERIAL) chunk_max = ((uint64_t)1 << 30) / (uint64_t)RW;
    const uint64_t chunk = std::min<uint64_t>(count, chunk_max);
    const int nch = (int)((count + chunk - 1) / chunk);
    const int nbuf = nch > 1 ? 2 : 1;
    if ((rc = ensure_cap(c, c->d_rec, c->rec_cap, chunk * RW * nbuf))) return rc;
    if ((rc = grow_events(c, c->phase_ev, 2 * (size_t)nch + 1))) return rc;
    if ((rc = grow_events(c, c->sync_ev, 2 * (size_t)nch))) return rc;
    if ((rc = ensure_packed(c))) return rc;
    const DevGraph dg = dev_graph(c);
    // hot/cold record split (C++ rules, hybrid): records touching no hot row
    // run through the plain-store kernel (train_draw.hip draw_split_kernel);
    // a study path, on with SMORE_SPLIT=1
    const bool split = mode == SMORE_HYBRID && !go && dg.vt32 && split_on();
    if (split && !c->d_split) HIPCHK(c, hipMalloc((void**)&c->d_split, 4 * sizeof(unsigned long long)));
    // tuning knob: SMORE_DRAW_LEAVE=0 keeps the update kernel's full grid
    // while the next chunk's draws run beside it
    const char* leave_env = getenv("SMORE_DRAW_LEAVE");
    const bool leave = !leave_env || atoi(leave_env) != 0;
    const int ugrid = nch > 1 ? edge_grid(c, fam, a, leave) : grid;
    hipStream_t ds = nch > 1 ? c->draw_stream : c->stream;
    auto recbuf = [&](int k) { return c->d_rec + (size_t)(k % nbuf) * chunk * RW; };
    auto draw = [&](int k) -> int {
        const uint64_t b = (uint64_t)k * chunk, n = std::min<uint64_t>(chunk, count - b);
        if (k >= 2) HIPCHK(c, hipStreamWaitEvent(ds, c->sync_ev[2 * (k - 2) + 1], 0));   // buffer free
        if (go) HIPCHK(c, launch_go_draw(dg, c->d_tcum, c->go_unit_w, seed, begin + b, n, a.K, recbuf(k), c->d_skipped, ds));
        else if (split) {
            unsigned long long* cnt = c->d_split + 2 * (k % nbuf);
            HIPCHK(c, hipMemsetAsync(cnt, 0, 2 * sizeof(unsigned long long), ds));
            HIPCHK(c, launch_draw_split(dg, seed, begin + b, n, a.K, alpha0, total,
                                        model == SMORE_MF || model == SMORE_BPR ? 0 : 1, recbuf(k), c->d_skipped, cnt,
                                        ds));
        } else HIPCHK(c, launch_draw(dg, seed, begin + b, n, a.K, recbuf(k), c->d_skipped, ds));
        HIPCHK(c, hipEventRecord(c->sync_ev[2 * k], ds));
        return SMORE_OK;
    };
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    HIPCHK(c, hipEventRecord(c->phase_ev[0], c->stream));
    if (ds != c->stream) HIPCHK(c, hipStreamWaitEvent(ds, c->phase_ev[0], 0));   // after earlier work
    if ((rc = draw(0))) return rc;
    for (int k = 0; k < nch; ++k) {
        if (k + 1 < nch && (rc = draw(k + 1))) return rc;
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->sync_ev[2 * k], 0));
        HIPCHK(c, hipEventRecord(c->phase_ev[2 * k + 1], c->stream));
        const uint64_t b = (uint64_t)k * chunk, n = std::min<uint64_t>(chunk, count - b);
        EdgeArgs ak = a;
        ak.begin = begin + b;
        ak.count = n;
        ak.rec = recbuf(k);
        HIPCHK(c, hipMemsetAsync(c->d_work, 0, sizeof(unsigned long long), c->stream));
        if (split) {
            // hot records [0, h) on the hybrid kernel, cold [h, n) on the
            // plain-store kernel; both read their rate from the record
            unsigned long long* cnt = c->d_split + 2 * (k % nbuf);
            ak.alpha_rec = 2;
            ak.count_dev = reinterpret_cast<const uint64_t*>(cnt);
            HIPCHK(c, launch_update(update_kernel(fam, ak), ak, ugrid, c->stream));
            EdgeArgs ac = ak;
            ac.mode = SMORE_HOGWILD;
            ac.sh_rows = 0;
            ac.count_dev = nullptr;
            ac.rec_base = reinterpret_cast<const uint64_t*>(cnt);
            HIPCHK(c, hipMemsetAsync(c->d_work, 0, sizeof(unsigned long long), c->stream));
            HIPCHK(c, launch_update(update_kernel(fam, ac), ac, edge_grid(c, fam, ac), c->stream));
        } else HIPCHK(c, launch_update(update_kernel(fam, ak), ak, ugrid, c->stream));
        HIPCHK(c, hipEventRecord(c->phase_ev[2 * k + 2], c->stream));
        HIPCHK(c, hipEventRecord(c->sync_ev[2 * k + 1], c->stream));
    }
    return finish_timed(c, mode, nch);
}

int smore_last_phase_ms(const smore_ctx* c, float* draw_ms, float* update_ms, int* launches) {
    if (!c || !c->timed || c->phase_n <= 0) return SMORE_ESTATE;
    float d = 0.0f, u = 0.0f, ms = 0.0f;
    if (hipEventSynchronize(c->phase_ev[2 * c->phase_n]) != hipSuccess) return SMORE_EHIP;
    for (int k = 0; k < c->phase_n; ++k) {
        if (hipEventElapsedTime(&ms, c->phase_ev[2 * k], c->phase_ev[2 * k + 1]) != hipSuccess) return SMORE_EHIP;
        d += ms;
        if (hipEventElapsedTime(&ms, c->phase_ev[2 * k + 1], c->phase_ev[2 * k + 2]) != hipSuccess) return SMORE_EHIP;
        u += ms;
    }
    if (draw_ms) *draw_ms = d;
    if (update_ms) *update_ms = u;
    if (launches) *launches = c->phase_n;
    return SMORE_OK;
}

int smore_train_edges(smore_ctx* c, int model, uint64_t begin, uint64_t count, uint64_t total, int K,
                      double alpha0, double reg, uint64_t seed, int mode) {
    return sync_after(c, smore_train_edges_async(c, model, begin, count, total, K, alpha0, reg, seed, mode), true);
}

int smore_sample_edges(smore_ctx* c, int model, uint64_t begin, uint64_t count, int K, uint64_t seed,
                       int32_t* out) {
    if (!c || !out) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (K < 0 || K > 20) return fail(c, SMORE_EINVAL, "bad K");
    if (count == 0) return SMORE_OK;
    int rc;
    if ((rc = set_device(c))) return rc;
    const int bpr = model == SMORE_BPR;
    const size_t width = c->semantics == SMORE_SEM_GO ? (bpr ? 3 : 2 + K) : (bpr ? 7 : 2 + K);
    int32_t* d = nullptr;
    HIPCHK(c, hipMalloc((void**)&d, count * width * sizeof(int32_t)));
    hipError_t e = c->semantics == SMORE_SEM_GO
                       ? launch_go_sample(dev_graph(c), c->d_tcum, seed, begin, count, bpr ? 1 : K, d, c->stream)
                       : launch_sample(dev_graph(c), seed, begin, count, K, bpr, d, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d, count * width * sizeof(int32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(c, SMORE_EHIP, std::string("sample: ") + hipGetErrorString(e));
    return SMORE_OK;
}

// Walk models on the record path: DeepWalk (rule 0) and Walklets (rule 1)
// walks -> skip-gram pair records -> update kernel.  `order` holds the walk
// start of every walk index (DeepWalk's shuffled keys; Walklets: vid).
// node2vec's device tables: the raw CSR edge weights (biasedTargetSample's
// base weights) and every vertex's CSR targets sorted (areNeighbors), built
// once per graph by all host threads.
static int ensure_n2v_tables(smore_ctx* c) {
    if (c->d_wts && c->d_nbr_sorted) return SMORE_OK;
    const HostGraph& g = *c->g;
    const int64_t V = g.V, E = g.E;
    std::vector<int32_t> nbr(g.targets.data(), g.targets.data() + E);
    const int nt = std::max(1, std::min(64, (int)std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t)
        th.emplace_back([&, t] {
            for (int64_t v = V * t / nt; v < V * (t + 1) / nt; ++v)
                std::sort(nbr.begin() + g.offsets[v], nbr.begin() + g.offsets[v + 1]);
        });
    for (auto& x : th) x.join();
    int rc;
    if ((rc = set_device(c))) return rc;
    if ((rc = upload(c, c->d_nbr_sorted, nbr.data(), nbr.size()))) return rc;
    return upload(c, c->d_wts, g.weights.data(), (size_t)E);
}

static int train_walks(smore_ctx* c, int rule, uint64_t walk_begin, uint64_t walk_end, int walk_times, int walk_steps,
                       int window, int window_min, int K, double alpha0, uint64_t seed, const int64_t* order,
                       uint64_t order_base, int mode, double n2v_p = 1.0, double n2v_q = 1.0,
                       int npaths = 0, double time_window = 0.0) {
    if (!c) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (c->ntables < 2) return fail(c, SMORE_ESTATE, "walk models need W and C tables");
    if (int rc_ = refuse_cse(c)) return rc_;
    if ((!order && rule != 1) || walk_times <= 0 || walk_steps < 0 || window <= 0 || K < 0 || K > 10 || mode < 0 || mode > 3)
        return fail(c, SMORE_EINVAL, "bad DeepWalk / Walklets arguments");
    if (rule == 1 && (window_min < 0 || window_min > window))
        return fail(c, SMORE_EINVAL, "Walklets: need 0 <= window_min <= window_max");
    if (rule == 1 && c->semantics == SMORE_SEM_GO) return fail(c, SMORE_EINVAL, "Walklets has no Go semantics");
    if (rule == 2 && c->semantics != SMORE_SEM_GO)
        return fail(c, SMORE_EINVAL, "node2vec is a Go model: smore_set_semantics(ctx, SMORE_SEM_GO) first");
    if (rule == 2 && !(n2v_p > 0 && n2v_q > 0)) return fail(c, SMORE_EINVAL, "node2vec: need p > 0 and q > 0");
    if (rule == 4 && c->semantics != SMORE_SEM_GO)
        return fail(c, SMORE_EINVAL, "CTDNE is a Go model: smore_set_semantics(ctx, SMORE_SEM_GO) first");
    if (rule == 4 && !c->has_temporal) return fail(c, SMORE_ESTATE, "CTDNE: no temporal edges");
    if (rule == 4 && time_window <= 0) time_window = (c->t_max_time - c->t_min_time) * 0.1;   // ctdne.go:45-49
    if (rule == 3 && c->semantics != SMORE_SEM_GO)
        return fail(c, SMORE_EINVAL, "metapath2vec is a Go model: smore_set_semantics(ctx, SMORE_SEM_GO) first");
    if (rule == 3 && (c->ntypes <= 0 || npaths <= 0 || !c->d_paths))
        return fail(c, SMORE_ESTATE, "metapath2vec: node types and meta-paths not set");
    const uint64_t total = (uint64_t)walk_times * (uint64_t)c->g->V;
    if (walk_end > total) walk_end = total;
    if (walk_begin >= walk_end) return SMORE_OK;
    // only this call's walks [walk_begin, walk_end) are read: validate and
    // upload that slice on every call (no caching by host pointer)
    const uint64_t nw_call = walk_end - walk_begin;
    int rc;
    if (order) {
        if (walk_begin < order_base) return fail(c, SMORE_EINVAL, "walk order slice does not cover the range");
        order -= order_base;   // order[w] is walk w's start
        for (uint64_t i = walk_begin; i < walk_end; ++i)
            if (order[i] < 0 || order[i] >= c->g->V) return fail(c, SMORE_EINVAL, "walk start out of range");
    }
    if ((rc = set_device(c))) return rc;
    if (rule == 2 && (rc = ensure_n2v_tables(c))) return rc;
    if (order) {   // else the starts are computed on the device (walk mod V)
        if ((rc = ensure_cap(c, c->d_order, c->order_cap, (size_t)nw_call))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->d_order, order + walk_begin, nw_call * sizeof(int64_t), hipMemcpyHostToDevice,
                                 c->stream));
    }
    // walks -> pair records -> update kernel (C++: edge_kernels.h over the
    // pair_emit records; Go: go_rec.h go_pair_kernel over go_pair_emit's);
    // chunks of up to 2^18 walks whose pair records (sized by the per-walk
    // upper bound, so no host read-back of the pair count) stay under 4 GiB
    const bool go = c->semantics == SMORE_SEM_GO;
    const int RW = rec_width(kmax_of(K));
    const uint64_t pb = std::max<uint64_t>(1, pair_bound(walk_steps, window, rule, window_min));
    uint64_t chunk_cap = (uint64_t)1 << 18;
    chunk_cap = std::max<uint64_t>(1, std::min<uint64_t>(chunk_cap, ((uint64_t)1 << 30) / (pb * RW)));
    const uint64_t chunk = std::min<uint64_t>(nw_call, chunk_cap);
    if ((rc = ensure_cap(c, c->d_walks, c->walk_buf_n, (size_t)chunk * (size_t)(walk_steps + 1)))) return rc;
    if ((rc = ensure_cap(c, c->d_lens, c->walk_lens_n, (size_t)chunk))) return rc;
    EdgeArgs a = record_args(c, SMORE_LINE2, K, mode);   // the walk kernels' (launch_go_walk)
    a.total = total;
    a.seed = seed;
    a.alpha0 = alpha0;
    // Go walks on a unit-weight graph: O(1) CDF target (go_target, tcum null)
    if (go && c->go_unit_w) a.tcum = nullptr;
    if (c->pair_walks < chunk + 1) {
        dfree(c->d_pcount);
        dfree(c->d_poff);
        c->pair_walks = 0;
        HIPCHK(c, hipMalloc((void**)&c->d_pcount, (chunk + 1) * sizeof(uint32_t)));
        HIPCHK(c, hipMalloc((void**)&c->d_poff, (chunk + 1) * sizeof(uint64_t)));
        c->pair_walks = chunk + 1;
    }
    if ((rc = ensure_cap(c, c->d_rec, c->rec_cap, (size_t)(chunk * pb * RW)))) return rc;
    // the update kernel over pair records; a stays the walk kernel's, taken
    // before the hot maps
    const UpdateFamily fam = go ? UpdateFamily::GoPair : UpdateFamily::Cpp;
    EdgeArgs ar;
    int ugrid;
    if ((rc = plan_pair_records(c, fam, K, mode, total, seed, alpha0, 0.0, chunk * pb, &ar, &ugrid))) return rc;
    ar.tcum = a.tcum;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (uint64_t b = walk_begin; b < walk_end; b += chunk) {
        WalkArgs w;
        w.order = order ? c->d_order : nullptr;
        w.order_base = walk_begin;
        w.walks = c->d_walks;
        w.lens = c->d_lens;
        w.walk_begin = b;
        w.nwalks = std::min<uint64_t>(chunk, walk_end - b);
        w.total_walks = total;
        w.steps = walk_steps;
        w.window = window;
        w.rule = rule;
        w.window_min = window_min;
        w.inv_p = 1.0 / n2v_p;   // node2vec.go:136,142 (fp64 1.0 / p)
        w.inv_q = 1.0 / n2v_q;
        w.wts = c->d_wts;
        w.nbr_sorted = c->d_nbr_sorted;
        w.ntype = c->d_ntype;
        w.ttargets = c->d_ttargets;
        w.toff = c->d_toff;
        w.paths = c->d_paths;
        w.path_off = c->d_path_off;
        w.ntypes = c->ntypes;
        w.npaths = npaths;
        w.slot_extra = rule >= 3 ? 1 : 0;   // metapath2vec: the path pick; CTDNE: the start time
        if (c->own_hi >= 0) {
            w.own_lo = (int32_t)c->own_lo;
            w.own_hi = (int32_t)c->own_hi;
        }
        // walks, then their pair counts plus a zero at n: the exclusive scan's
        // entry n is the chunk's pair total, which the update kernel reads on
        // the device (no host round trip between chunks)
        if (rule == 4) {
            TemporalArgs tg{c->d_t_off, c->d_t_tgt, c->d_t_ts, c->d_t_min, c->d_t_max, c->t_max_time, time_window};
            HIPCHK(c, launch_go_ctdne_walk(tg, w, seed, c->stream));
        } else if (go) {
            HIPCHK(c, launch_go_walk(a, w, 1, c->stream));
        } else {
            HIPCHK(c, launch_walk_gen(ar.g, w, seed, c->stream));
        }
        HIPCHK(c, hipMemsetAsync(c->d_pcount + w.nwalks, 0, sizeof(uint32_t), c->stream));
        if (go) HIPCHK(c, launch_go_pair_count(w, c->d_pcount, c->stream));
        else HIPCHK(c, launch_pair_count(w, seed, c->d_pcount, c->stream));
        HIPCHK(c, scan_pair_counts(c->d_pcount, c->d_poff, w.nwalks + 1, &c->d_scan_tmp, &c->scan_tmp_bytes,
                                   c->stream));
        if (go)
            HIPCHK(c, launch_go_pair_emit(ar.g, w, seed, K, alpha0, c->d_poff, c->d_rec, mode == SMORE_HYBRID,
                                          c->stream));
        else HIPCHK(c, launch_pair_emit(ar.g, w, seed, K, alpha0, c->d_poff, c->d_rec, c->stream));
        EdgeArgs ak = ar;
        ak.begin = 0;
        ak.count = w.nwalks * pb;
        ak.count_dev = c->d_poff + w.nwalks;
        if ((rc = launch_record_update(c, fam, ak, ugrid))) return rc;
    }
    return finish_timed(c, mode, 0);
}

int smore_train_deepwalk_async(smore_ctx* c, uint64_t walk_begin, uint64_t walk_end, int walk_times,
                               int walk_steps, int window, int K, double alpha0, uint64_t seed, const int64_t* order,
                               int mode) {
    return train_walks(c, 0, walk_begin, walk_end, walk_times, walk_steps, window, 0, K, alpha0, seed, order, 0,
                       mode);
}

int smore_train_node2vec_async(smore_ctx* c, uint64_t walk_begin, uint64_t walk_end, int walk_times,
                               int walk_steps, int window, int K, double alpha0, double p, double q, uint64_t seed,
                               const int64_t* order, int mode) {
    return train_walks(c, 2, walk_begin, walk_end, walk_times, walk_steps, window, 0, K, alpha0, seed, order, 0, mode,
                       p, q);
}

int smore_train_metapath2vec_async(smore_ctx* c, uint64_t walk_begin, uint64_t walk_end, int walk_times,
                                   int walk_steps, int window, int K, double alpha0, const int32_t* paths,
                                   const int32_t* path_lens, int npaths, uint64_t seed, const int64_t* order,
                                   int mode) {
    if (!c) return SMORE_EINVAL;
    if (!paths || !path_lens || npaths <= 0) return fail(c, SMORE_EINVAL, "metapath2vec: no meta-paths");
    std::vector<int32_t> off((size_t)npaths + 1, 0);
    for (int p = 0; p < npaths; ++p) {
        if (path_lens[p] < 0) return fail(c, SMORE_EINVAL, "metapath2vec: bad path length");
        off[p + 1] = off[p] + path_lens[p];
    }
    for (int32_t i = 0; i < off[npaths]; ++i)
        if (paths[i] < 0 || paths[i] >= c->ntypes) return fail(c, SMORE_EINVAL, "metapath2vec: unknown type in path");
    int rc;
    if ((rc = set_device(c))) return rc;
    std::vector<int32_t> key(path_lens, path_lens + npaths);
    key.insert(key.end(), paths, paths + off[npaths]);
    if (key != c->path_host || !c->d_paths) {
        // the previous call's kernels may still read the paths: reallocate
        // only after the stream has drained
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if ((rc = upload(c, c->d_paths, paths, (size_t)off[npaths]))) return rc;
        if ((rc = upload(c, c->d_path_off, off.data(), off.size()))) return rc;
        c->path_host.swap(key);
    }
    return train_walks(c, 3, walk_begin, walk_end, walk_times, walk_steps, window, 0, K, alpha0, seed, order, 0, mode,
                       1.0, 1.0, npaths);
}

int smore_train_metapath2vec(smore_ctx* c, uint64_t walk_begin, uint64_t walk_end, int walk_times, int walk_steps,
                             int window, int K, double alpha0, const int32_t* paths, const int32_t* path_lens,
                             int npaths, uint64_t seed, const int64_t* order, int mode) {
    int rc = smore_train_metapath2vec_async(c, walk_begin, walk_end, walk_times, walk_steps, window, K, alpha0, paths,
                                            path_lens, npaths, seed, order, mode);
    return sync_after(c, rc);
}

int smore_train_ctdne_async(smore_ctx* c, uint64_t walk_begin, uint64_t walk_end, int walk_times, int walk_steps,
                            int window, int K, double alpha0, double time_window, uint64_t seed, const int64_t* order,
                            int mode) {
    return train_walks(c, 4, walk_begin, walk_end, walk_times, walk_steps, window, 0, K, alpha0, seed, order, 0, mode,
                       1.0, 1.0, 0, time_window);
}

int smore_train_ctdne(smore_ctx* c, uint64_t walk_begin, uint64_t walk_end, int walk_times, int walk_steps, int window,
                      int K, double alpha0, double time_window, uint64_t seed, const int64_t* order, int mode) {
    int rc = smore_train_ctdne_async(c, walk_begin, walk_end, walk_times, walk_steps, window, K, alpha0, time_window,
                                     seed, order, mode);
    return sync_after(c, rc);
}

int smore_train_node2vec(smore_ctx* c, uint64_t walk_begin, uint64_t walk_end, int walk_times, int walk_steps,
                         int window, int K, double alpha0, double p, double q, uint64_t seed, const int64_t* order,
                         int mode) {
    int rc = smore_train_node2vec_async(c, walk_begin, walk_end, walk_times, walk_steps, window, K, alpha0, p, q,
                                        seed, order, mode);
    return sync_after(c, rc);
}

int smore_train_walklets_async(smore_ctx* c, uint64_t walk_begin, uint64_t walk_end, int walk_times, int walk_steps,
                               int window_min, int window_max, int K, double alpha0, uint64_t seed, int mode) {
    if (!c) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (walk_times <= 0) return fail(c, SMORE_EINVAL, "bad DeepWalk / Walklets arguments");
    // Walklets::Train walks from vid itself (src/model/Walklets.cpp:45): no
    // order array, the walk kernel starts walk w at w mod V
    return train_walks(c, 1, walk_begin, walk_end, walk_times, walk_steps, window_max, window_min, K, alpha0, seed,
                       nullptr, 0, mode);
}

int smore_train_walklets(smore_ctx* c, uint64_t walk_begin, uint64_t walk_end, int walk_times, int walk_steps,
                         int window_min, int window_max, int K, double alpha0, uint64_t seed, int mode) {
    int rc = smore_train_walklets_async(c, walk_begin, walk_end, walk_times, walk_steps, window_min, window_max, K,
                                        alpha0, seed, mode);
    return sync_after(c, rc);
}

int smore_train_app_async(smore_ctx* c, uint64_t unit_begin, uint64_t unit_end, int walk_times, int sample_times,
                          double jump, int K, double alpha0, uint64_t seed, const int64_t* order, int mode) {
    if (!c) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (c->ntables < 2) return fail(c, SMORE_ESTATE, "APP needs W and C tables");
    if (int rc_ = refuse_cse(c)) return rc_;
    if (c->semantics == SMORE_SEM_GO) return fail(c, SMORE_EINVAL, "APP has no Go semantics");
    // jump <= 0 never ends a walk on a graph without dead ends (the reference
    // loops forever); the device walk is bounded, but reject it up front
    if (!order || walk_times <= 0 || sample_times <= 0 || !(jump > 0.0) || K < 0 || K > 10 || mode < 0 || mode > 3)
        return fail(c, SMORE_EINVAL, "bad APP arguments");
    const uint64_t total = (uint64_t)walk_times * (uint64_t)c->g->V;
    const uint64_t units = total * (uint64_t)sample_times;
    if (unit_end > units) unit_end = units;
    if (unit_begin >= unit_end) return SMORE_OK;
    const uint64_t w0 = unit_begin / (uint64_t)sample_times, w1 = (unit_end - 1) / (uint64_t)sample_times + 1;
    for (uint64_t w = w0; w < w1; ++w)
        if (order[w] < 0 || order[w] >= c->g->V) return fail(c, SMORE_EINVAL, "walk start out of range");
    int rc;
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure_cap(c, c->d_order, c->order_cap, (size_t)(w1 - w0)))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_order, order + w0, (w1 - w0) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    const int RW = rec_width(kmax_of(K));
    const uint64_t chunk = std::min<uint64_t>(unit_end - unit_begin, (uint64_t)1 << 25);
    if ((rc = ensure_cap(c, c->d_rec, c->rec_cap, (size_t)(chunk * RW)))) return rc;
    EdgeArgs a;
    int grid;
    if ((rc = plan_pair_records(c, UpdateFamily::Cpp, K, mode, total, seed, alpha0, 0.0, chunk, &a, &grid))) return rc;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (uint64_t b = unit_begin; b < unit_end; b += chunk) {
        AppArgs p;
        p.order = c->d_order;
        p.order_base = w0;
        p.unit_begin = b;
        p.n = std::min<uint64_t>(chunk, unit_end - b);
        p.total_walks = total;
        p.sample_times = sample_times;
        p.jump = jump;
        HIPCHK(c, launch_app_records(a.g, p, seed, K, alpha0, c->d_rec, c->stream));
        EdgeArgs ak = a;
        ak.begin = 0;
        ak.count = p.n;
        if ((rc = launch_record_update(c, UpdateFamily::Cpp, ak, grid))) return rc;
    }
    return finish_timed(c, mode, 0);
}

int smore_train_app(smore_ctx* c, uint64_t unit_begin, uint64_t unit_end, int walk_times, int sample_times,
                    double jump, int K, double alpha0, uint64_t seed, const int64_t* order, int mode) {
    int rc = smore_train_app_async(c, unit_begin, unit_end, walk_times, sample_times, jump, K, alpha0, seed, order,
                                   mode);
    return sync_after(c, rc);
}

int smore_train_hpe_async(smore_ctx* c, uint64_t begin, uint64_t count, uint64_t total, int walk_steps, int K,
                          double reg, double alpha0, uint64_t seed, int mode) {
    if (!c) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (c->ntables < 2) return fail(c, SMORE_ESTATE, "HPE needs W and C tables");
    if (int rc_ = refuse_cse(c)) return rc_;
    if (c->semantics == SMORE_SEM_GO) return fail(c, SMORE_EINVAL, "HPE in Go semantics is the Go LINE-2 rule (internal/models/hpe/hpe.go:72-124): smore_train_edges with SMORE_LINE2");
    if (walk_steps < 1 || walk_steps > 4096 || K < 0 || K > 10 || mode < 0 || mode > 3 || total == 0)
        return fail(c, SMORE_EINVAL, "bad HPE arguments");
    if (count == 0) return SMORE_OK;
    int rc;
    if ((rc = set_device(c))) return rc;
    const int RW = rec_width(kmax_of(K));
    const uint64_t nrec = (uint64_t)walk_steps + 1;
    const uint64_t chunk = std::min<uint64_t>(count, std::max<uint64_t>(1, ((uint64_t)1 << 27) / nrec));
    if ((rc = ensure_cap(c, c->d_rec, c->rec_cap, (size_t)(chunk * nrec * RW)))) return rc;
    EdgeArgs a;
    int grid;
    if ((rc = plan_pair_records(c, UpdateFamily::Cpp, K, mode, total, seed, alpha0, reg, chunk * nrec, &a, &grid)))
        return rc;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (uint64_t b = begin; b < begin + count; b += chunk) {
        HpeArgs p;
        p.begin = b;
        p.n = std::min<uint64_t>(chunk, begin + count - b);
        p.total = total;
        p.walk_steps = walk_steps;
        HIPCHK(c, launch_hpe_records(a.g, p, seed, K, alpha0, c->d_rec, c->d_skipped, c->stream));
        EdgeArgs ak = a;
        ak.begin = 0;
        ak.count = p.n * nrec;
        if ((rc = launch_record_update(c, UpdateFamily::Cpp, ak, grid))) return rc;
    }
    return finish_timed(c, mode, 0);
}

int smore_train_hpe(smore_ctx* c, uint64_t begin, uint64_t count, uint64_t total, int walk_steps, int K, double reg,
                    double alpha0, uint64_t seed, int mode) {
    int rc = smore_train_hpe_async(c, begin, count, total, walk_steps, K, reg, alpha0, seed, mode);
    return sync_after(c, rc);
}

int smore_train_deepwalk(smore_ctx* c, uint64_t walk_begin, uint64_t walk_end, int walk_times, int walk_steps,
                         int window, int K, double alpha0, uint64_t seed, const int64_t* order, int mode) {
    int rc = smore_train_deepwalk_async(c, walk_begin, walk_end, walk_times, walk_steps, window, K, alpha0, seed,
                                        order, mode);
    return sync_after(c, rc);
}

}  // extern "C"

// ---------------------------------------------------------------- caller pairs
// proNet::UpdatePairs (src/proNet.cpp:2741-2753) / Go (*ProNet).UpdatePairs
// (pkg/pronet/optimizer.go:8-18): the caller's pairs become records
// (caller_pair_kernel, negatives drawn on the device) for the pair kernels --
// pair_train_kernel (C++ UpdatePair; serial: edge_train_kernel's in-order
// path) or go_pair_kernel (Go UpdatePair) -- in chunks of up to 2^24 pairs.
// smore_train_pairs queued on the stream (the caller synchronizes)
int smore_host::train_pairs_core(smore_ctx* c, const int32_t* v, const int32_t* cc, int64_t n, int K, double alpha,
                                 uint64_t seed, uint64_t unit, int mode) {
    if (!c) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (c->ntables < 2) return fail(c, SMORE_ESTATE, "UpdatePairs needs W and C tables");
    if (int rc_ = refuse_cse(c)) return rc_;
    if (n < 0 || (n > 0 && (!v || !cc)) || K < 0 || K > 10 || mode < 0 || mode > 3)
        return fail(c, SMORE_EINVAL, "bad UpdatePairs arguments");
    if (n == 0) return SMORE_OK;
    const int64_t V = c->g->V;
    for (int64_t i = 0; i < n; ++i)
        if (v[i] < 0 || v[i] >= V || cc[i] < 0 || cc[i] >= V) return fail(c, SMORE_EINVAL, "pair id out of range");
    int rc;
    if ((rc = set_device(c))) return rc;
    const bool go = c->semantics == SMORE_SEM_GO;
    const int RW = rec_width(kmax_of(K));
    const uint64_t chunk = std::min<uint64_t>((uint64_t)n, (uint64_t)1 << 24);
    // (v, c) halves of `chunk` ids each; earlier calls' kernels may still read
    // either buffer: growing frees it, and the free waits for the device
    if ((rc = ensure_cap(c, c->d_pairs, c->pairs_cap, (size_t)(2 * chunk)))) return rc;
    if ((rc = ensure_cap(c, c->d_rec, c->rec_cap, (size_t)(chunk * RW)))) return rc;
    const UpdateFamily fam = go ? UpdateFamily::GoPair : UpdateFamily::Cpp;
    EdgeArgs a;
    int grid;
    if ((rc = plan_pair_records(c, fam, K, mode, 1, seed, alpha, 0.0, chunk, &a, &grid))) return rc;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (uint64_t b = 0; b < (uint64_t)n; b += chunk) {
        const uint64_t m = std::min<uint64_t>(chunk, (uint64_t)n - b);
        // the previous chunk's kernels read d_pairs / d_rec: the copies are
        // ordered after them on the stream
        HIPCHK(c, hipMemcpyAsync(c->d_pairs, v + b, m * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_pairs + chunk, cc + b, m * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, launch_caller_pairs(a.g, c->d_pairs, c->d_pairs + chunk, m, b, K, (float)alpha, seed, unit, go ? 1 : 0,
                                      mode == SMORE_HYBRID, c->d_rec, c->stream));
        EdgeArgs ak = a;
        ak.begin = 0;
        ak.count = m;
        // a small batch (one walk's pairs, the Go callers' unit): short
        // slices so that every pair gets a group of its own; the
        // CH_ROUNDS-record slices keep W_v in registers over a long batch
        const uint64_t groups = (uint64_t)grid * (uint64_t)(256 / lanes_of(c->dpad));
        if (m < groups * CH_ROUNDS) ak.pair_slice = (uint32_t)std::max<uint64_t>(1, (m + groups - 1) / groups);
        if ((rc = launch_record_update(c, fam, ak, grid))) return rc;
    }
    return finish_timed(c, mode, 0);
}

extern "C" {

int smore_train_pairs(smore_ctx* c, const int32_t* v, const int32_t* cc, int64_t n, int K, double alpha,
                      uint64_t seed, uint64_t unit, int mode) {
    int rc = train_pairs_core(c, v, cc, n, K, alpha, seed, unit, mode);
    if (rc || !c || n == 0) return rc;
    return sync_after(c, rc, true);
}

}  // extern "C"

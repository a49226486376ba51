// group.cpp -- one process, N GPUs: the smore_group_* calls of the C ABI.  A
// group holds one context per replica; its collectives go out as one grouped
// RCCL call (or, with every replica on one device, as device passes), and a
// training call runs either the replica schedule (group_rounds: every replica
// trains a slice of each round, table deltas exchanged through exchange.cpp)
// or the 2-D block schedule (group_blocks.cpp).
#include <initializer_list>

#include "group.h"
#include "hot_exchange.h"

using namespace smore_host;

namespace smore_host {

// ---- the group's collectives over per-replica buffers, each replica's part
// on its own stream (RCCL: one grouped call; local: device passes)
int coll_allreduce(smore_group* g, const std::vector<float*>& buf, size_t n, const std::vector<hipStream_t>& st,
                   const char* what) {
    const size_t R = g->ctx.size();
    if (g->local) {
        smore_ctx* c0 = g->ctx[0];
        int rc;
        if ((rc = set_device(c0))) return gfail(g, 0, rc);
        // the sum runs on replica 0's stream after every replica's stream
        // reached this point; every stream continues after the sum
        for (size_t r = 1; r < R; ++r) {
            if (hipEventRecord(g->lev[r], st[r]) != hipSuccess || hipStreamWaitEvent(st[0], g->lev[r], 0) != hipSuccess)
                return gfail(g, (int)r, fail(g->ctx[r], SMORE_EHIP, std::string(what) + ": event"));
        }
        if (launch_local_sum(buf.data(), (int)R, n, c0->cus, st[0]) != hipSuccess)
            return gfail(g, 0, fail(c0, SMORE_EHIP, std::string(what) + ": local sum"));
        if (hipEventRecord(g->ldone, st[0]) != hipSuccess) return gfail(g, 0, fail(c0, SMORE_EHIP, what));
        for (size_t r = 1; r < R; ++r)
            if (hipStreamWaitEvent(st[r], g->ldone, 0) != hipSuccess)
                return gfail(g, (int)r, fail(g->ctx[r], SMORE_EHIP, what));
        return SMORE_OK;
    }
    Rccl* L = rccl();
    ncclResult_t nr = L->group_start();
    for (size_t r = 0; r < R && nr == ncclSuccess; ++r) {
        (void)hipSetDevice(g->ctx[r]->device);
        nr = L->all_reduce(buf[r], buf[r], n, ncclFloat32, ncclSum, (ncclComm_t)g->ctx[r]->comm, st[r]);
    }
    ncclResult_t ne = L->group_end();
    if (nr == ncclSuccess) nr = ne;
    if (nr != ncclSuccess) return gfail(g, 0, nccl_fail(g->ctx[0], what, nr));
    return SMORE_OK;
}

int coll_broadcast(smore_group* g, const std::vector<float*>& buf, size_t n, int root,
                   const std::vector<hipStream_t>& st, const char* what) {
    const size_t R = g->ctx.size();
    if (g->local) {
        int rc;
        if ((rc = set_device(g->ctx[0]))) return gfail(g, 0, rc);
        if (hipEventRecord(g->ldone, st[root]) != hipSuccess) return gfail(g, root, fail(g->ctx[root], SMORE_EHIP, what));
        for (size_t r = 0; r < R; ++r) {
            if ((int)r == root) continue;
            // the copy waits for the root's stream; the root's stream waits
            // for the copy before it writes the rows again
            if (hipStreamWaitEvent(st[r], g->ldone, 0) != hipSuccess ||
                hipMemcpyAsync(buf[r], buf[root], n * sizeof(float), hipMemcpyDeviceToDevice, st[r]) != hipSuccess ||
                hipEventRecord(g->lev[r], st[r]) != hipSuccess || hipStreamWaitEvent(st[root], g->lev[r], 0) != hipSuccess)
                return gfail(g, (int)r, fail(g->ctx[r], SMORE_EHIP, std::string(what) + ": local copy"));
        }
        return SMORE_OK;
    }
    Rccl* L = rccl();
    ncclResult_t nr = L->group_start();
    for (size_t r = 0; r < R && nr == ncclSuccess; ++r) {
        (void)hipSetDevice(g->ctx[r]->device);
        nr = L->broadcast(buf[r], buf[r], n, ncclFloat32, root, (ncclComm_t)g->ctx[r]->comm, st[r]);
    }
    ncclResult_t ne = L->group_end();
    if (nr == ncclSuccess) nr = ne;
    if (nr != ncclSuccess) return gfail(g, 0, nccl_fail(g->ctx[0], what, nr));
    return SMORE_OK;
}

std::vector<hipStream_t> compute_streams(const smore_group* g) {
    std::vector<hipStream_t> st;
    for (smore_ctx* c : g->ctx) st.push_back(c->stream);
    return st;
}

// every replica adopts replica 0's (shared) host graph and uploads it
static int replicate_graph(smore_group* g) {
    smore_ctx* c0 = g->ctx[0];
    for (size_t r = 1; r < g->ctx.size(); ++r) {
        smore_ctx* c = g->ctx[r];
        c->g = c0->g;
        c->hot_key.clear();
        c->semantics = SMORE_SEM_CPP;
        int rc = upload_graph(c);
        if (rc) return gfail(g, (int)r, rc);
    }
    return SMORE_OK;
}

static int group_exchange_begin(smore_group* g, int rule) {
    int rc;
    const size_t R = g->ctx.size();
    for (size_t r = 0; r < R; ++r)
        if ((rc = exchange_passes(g->ctx[r], rule))) return gfail(g, (int)r, rc);
    std::vector<hipStream_t> st;
    for (smore_ctx* c : g->ctx) st.push_back(c->comm_stream);
    for (int t = g->ctx[0]->ex_t0; t < g->ctx[0]->ntables; ++t) {
        std::vector<float*> buf;
        for (smore_ctx* c : g->ctx) buf.push_back(c->ex_buf[t][2]);
        if ((rc = coll_allreduce(g, buf, g->ctx[0]->ex_n, st, "ncclAllReduce"))) return rc;
    }
    for (size_t r = 0; r < R; ++r)
        if ((rc = exchange_posted(g->ctx[r]))) return gfail(g, (int)r, rc);
    return SMORE_OK;
}

// the hub rows of every exchanged table of every replica (replica 0's host
// graph: all replicas share it); keyed by the rows' law and the tables (the
// key is cleared with the graph, upload_graph)
static int ensure_hot(smore_group* g, int model, int K, int64_t rows) {
    smore_ctx* c0 = g->ctx[0];
    const std::string key = std::to_string(model) + "/" + std::to_string(K) + "/" + std::to_string(rows) + "/" +
                            std::to_string(c0->dpad) + "/" + std::to_string(c0->ntables) + "/" +
                            std::to_string(c0->ex_t0) + "/" + std::to_string(c0->g->V) + "/" +
                            std::to_string(c0->g->E) + "/" + c0->census_key;
    bool same = true;
    for (smore_ctx* c : g->ctx) same = same && c->hot_ex_key == key;
    if (same) return SMORE_OK;
    std::vector<int32_t> ids[2];
    for (int t = c0->ex_t0; t < c0->ntables; ++t) {
        ids[t].resize((size_t)rows);
        int rc = smore_hot_row_ids(c0, model, K, t, rows, ids[t].data());
        if (rc) return gfail(g, 0, rc);
    }
    for (size_t r = 0; r < g->ctx.size(); ++r) {
        smore_ctx* c = g->ctx[r];
        int rc;
        if ((rc = set_device(c))) return gfail(g, (int)r, rc);
        for (int t = 0; t < 2; ++t) {
            dfree(c->hot_idx[t]);
            dfree(c->hot_buf[t][0]);
            dfree(c->hot_buf[t][1]);
        }
        for (int t = c->ex_t0; t < c->ntables; ++t) {
            if ((rc = upload(c, c->hot_idx[t], ids[t].data(), ids[t].size()))) return gfail(g, (int)r, rc);
            for (float*& p : c->hot_buf[t])
                if (hipMalloc((void**)&p, (size_t)rows * c->dpad * sizeof(float)) != hipSuccess)
                    return gfail(g, (int)r, fail(c, SMORE_EHIP, "hub-row exchange buffers"));
        }
        c->hot_n = rows;
        c->hot_ex_key = key;
    }
    return SMORE_OK;
}

// the synchronous hub-row exchange of the exchanged tables on every replica's
// compute stream (a table outside [ex_t0, ntables) has no snapshot to pack against)
static int group_hot_exchange(smore_group* g) {
    int rc;
    const int t0 = g->ctx[0]->ex_t0;
    for (size_t r = 0; r < g->ctx.size(); ++r) {
        smore_ctx* c = g->ctx[r];
        if ((rc = set_device(c))) return gfail(g, (int)r, rc);
        for (int t = t0; t < c->ntables; ++t)
            if (launch_hot_pack(c->d_table[t], c->ex_buf[t][0], c->hot_idx[t], (uint64_t)c->hot_n, c->dpad,
                                c->hot_buf[t][0], c->hot_buf[t][1], c->cus, c->stream) != hipSuccess)
                return gfail(g, (int)r, fail(c, SMORE_EHIP, "hot_pack"));
    }
    const std::vector<hipStream_t> st = compute_streams(g);
    for (int t = t0; t < g->ctx[0]->ntables; ++t) {
        std::vector<float*> buf;
        for (smore_ctx* c : g->ctx) buf.push_back(c->hot_buf[t][1]);
        if ((rc = coll_allreduce(g, buf, (size_t)g->ctx[0]->hot_n * g->ctx[0]->dpad, st, "hub-row ncclAllReduce")))
            return rc;
    }
    for (size_t r = 0; r < g->ctx.size(); ++r) {
        smore_ctx* c = g->ctx[r];
        if ((rc = set_device(c))) return gfail(g, (int)r, rc);
        for (int t = t0; t < c->ntables; ++t)
            if (launch_hot_unpack(c->d_table[t], c->ex_buf[t][0], c->hot_idx[t], (uint64_t)c->hot_n, c->dpad,
                                  c->hot_buf[t][0], c->hot_buf[t][1], c->cus, c->stream) != hipSuccess)
                return gfail(g, (int)r, fail(c, SMORE_EHIP, "hot_unpack"));
    }
    return SMORE_OK;
}

// every replica gets every part's W rows from the part's owner (replica p
// owns rows [b[p], b[p+1]): the source partition's or the walk partition's
// parts): one in-place broadcast per part
static int gather_sources(smore_group* g, const std::vector<int64_t>& b) {
    const size_t n = g->ctx.size();
    int rc;
    const std::vector<hipStream_t> st = compute_streams(g);
    for (size_t p = 0; p < n; ++p) {
        if (b[p + 1] <= b[p]) continue;
        std::vector<float*> rows;
        for (smore_ctx* c : g->ctx) rows.push_back(c->d_table[0] + (size_t)b[p] * c->dpad);
        if ((rc = coll_broadcast(g, rows, (size_t)(b[p + 1] - b[p]) * g->ctx[0]->dpad, (int)p, st,
                                 "W gather ncclBroadcast")))
            return rc;
    }
    return SMORE_OK;
}

// the end of a group call: with RCCL communicators the host waits for every
// replica's stream under the failure watch (comm_watch.h: async errors
// polled, the wait bounded, communicators aborted on failure)
int group_sync(smore_group* g) {
    int rc;
    if (!g->local && !g->comms.empty()) {
        std::string why;
        int bad = -1;
        auto ready = [&]() -> int {
            for (size_t r = 0; r < g->ctx.size(); ++r) {
                (void)hipSetDevice(g->ctx[r]->device);
                const hipError_t e = hipStreamQuery(g->ctx[r]->stream);
                if (e == hipErrorNotReady) return 0;
                if (e != hipSuccess) {
                    bad = (int)r;
                    return -1;
                }
            }
            return 1;
        };
        if (comm_watch(rccl(), g->comms.data(), (int)g->comms.size(), ready, comm_timeout(), why)) {
            // the communicators are aborted (freed): no replica may use its
            // handle again, and the group's teardown skips them
            for (smore_ctx* c : g->ctx) c->comm = nullptr;
            return gfail(g, bad < 0 ? 0 : bad, fail(g->ctx[bad < 0 ? 0 : bad], SMORE_EHIP, why));
        }
    }
    for (size_t r = 0; r < g->ctx.size(); ++r)
        if ((rc = smore_synchronize(g->ctx[r]))) return gfail(g, (int)r, rc);
    return SMORE_OK;
}

}  // namespace smore_host

// The group training round structure.  The range [begin, end) is cut into
// R = ceil(count / (per * N)) rounds of equal size (+-1); round k's units are
// split evenly over the N replicas (replica r gets the r-th of N equal
// slices, so every replica trains a share of every call -- with the source
// partition a replica that got nothing would leave its part's W rows
// untrained).  Replica r queues its slice on its stream (run(ctx, b, e) must
// not synchronize), then the group folds the previous exchange in and starts
// this round's all-reduce, which overlaps round k+1.  rule: SMORE_SYNC_*; the
// adaptive rule's row scales are made for `model` with K negatives at the
// replicas' actual units per round (count / (R N)) * upu updates per replica
// per exchange (upu: updates per unit).  model SMORE_CENSUS (the walk models):
// the rows' touches per unit come from a census of the call's first round on
// replica 0 (run in census mode: records generated, rows counted, nothing
// trained; smore_census_begin), redone only when census_key changes.  With
// the hub-row exchange on (sum rule), each replica's slice runs as
// g->launches launches and the hub rows are synced after each.
//
// part (LINE-2): the source partition.  walkpart (the walk models whose pairs
// come from pair_emit / go_pair_emit): the walk partition -- every replica
// runs the whole round and trains the pairs whose center it owns
// (smore_set_walk_owner over smore_walk_parts of the census), only C is
// exchanged, W is gathered from the owners at the end.
// Default exchange periods (per = 0): measured on config 2's graph for LINE-2
// (tools/replica_study.py + tools/samples_to_loss.py: 6.7 samples per row per
// replica per exchange gives the best effective 8-GPU speed-up, 4.4-5.4x
// counting the exchange passes; 13.4: 3.7-5.1x) and on config 5's for
// DeepWalk (4 pair updates per row per replica, c0 64: 1.02 / 1.07 / 1.35x
// one replica's held-out loss at 2 / 4 / 8 replicas; 54, about the old 2^18
// walks, drain 32: 1.09 / 1.79 / 3.75x), profiles/r04/replica
constexpr double EDGE_PER_ROW = 6.71, EDGE_PER_MIN = 4096.0, EDGE_PER_MAX = 134217728.0, WALK_PER_ROW = 4.0;

template <class F>
static int group_rounds(smore_group* g, uint64_t begin, uint64_t end, uint64_t per, int rule, F&& run,
                        int model = SMORE_LINE2, int K = 5, double upu = 1.0, bool part = false,
                        const std::string& census_key = std::string(), bool walkpart = false) {
    const size_t n = g->ctx.size();
    int rc;
    if (end <= begin) return SMORE_OK;
    if (rule < SMORE_SYNC_SUM || rule > SMORE_SYNC_ADAPTIVE) return gfail(g, 0, fail(g->ctx[0], SMORE_EINVAL, "bad exchange rule"));
    // LINE-2 with the source partition: replica r draws its sources from part
    // r, owns those W rows, and only C is exchanged (W gathered at the end)
    part = part && g->partition && n > 1;
    walkpart = walkpart && !part && g->walk_partition && n > 1;
    for (size_t r = 0; r < n; ++r) {
        smore_ctx* c = g->ctx[r];
        if ((rc = smore_set_source_partition(c, part ? (int)n : 1, part ? (int)r : 0))) return gfail(g, (int)r, rc);
        if ((rc = smore_set_walk_owner(c, 0, -1))) return gfail(g, (int)r, rc);
        c->ex_t0 = part || walkpart ? 1 : 0;
        if ((rc = exchange_reset(c))) return gfail(g, (int)r, rc);
    }
    const uint64_t count = end - begin;
    int64_t rows = g->hot_rows < 0 ? std::min<int64_t>(65536, g->ctx[0]->g->V / 8) : g->hot_rows;
    rows = std::min<int64_t>(rows, g->ctx[0]->g->V);
    const bool hot = rule == SMORE_SYNC_SUM && rows > 0 && g->launches > 1;
    const int64_t V = g->ctx[0]->g->V;
    if (model == SMORE_CENSUS && (rule == SMORE_SYNC_ADAPTIVE || hot || walkpart || per == 0)) {
        smore_ctx* c0 = g->ctx[0];
        const std::string key = census_key + "/" + std::to_string(c0->semantics);
        if (c0->census_key != key || !c0->census_ok) {
            // the first round (or 2^16 units at least, so that the hub rows'
            // rates are well measured on small rounds, or the call)
            const uint64_t m = std::min<uint64_t>(count, std::max<uint64_t>(per * (uint64_t)n, (uint64_t)1 << 16));
            if ((rc = smore_census_begin(c0))) return gfail(g, 0, rc);
            // m units in 16 slices spread evenly over [begin, end), not the
            // leading m: walks without a start order begin at walk mod V, so a
            // prefix would census one contiguous id block's neighbourhood only
            // 
            const uint64_t ns = std::min<uint64_t>(16, m);
            rc = SMORE_OK;
            for (uint64_t k = 0; k < ns && !rc; ++k) {
                const uint64_t lo = begin + (uint64_t)(((unsigned __int128)count * k) / ns);
                const uint64_t len = m * (k + 1) / ns - m * k / ns;
                if (len) rc = run(c0, lo, lo + len);
            }
            const int rc2 = smore_census_end(c0, (double)m);
            if (rc || rc2) return gfail(g, 0, rc ? rc : rc2);
            c0->census_key = key;
            for (size_t r = 1; r < n; ++r) g->ctx[r]->census_key.clear();
        }
    }
    if (per == 0) {
        // the default exchange period, relative to the graph:
        // edge models EDGE_PER_ROW samples per row per replica, walk models
        // WALK_PER_ROW W updates (pairs) per row per replica, from the census
        if (model == SMORE_CENSUS) {
            double upr = 0.0;   // W touches (pairs) per unit
            for (double x : g->ctx[0]->census_rate[0]) upr += x;
            per = (uint64_t)std::max(1.0, std::round(WALK_PER_ROW * (double)V / std::max(upr, 1e-30)));
        } else {
            per = (uint64_t)std::min(EDGE_PER_MAX, std::max(EDGE_PER_MIN, std::round(EDGE_PER_ROW * (double)V)));
        }
    }
    const uint64_t round_units = per > count / n ? count : per * (uint64_t)n;   // no overflow: per * n <= count
    const uint64_t rounds = (count + round_units - 1) / round_units;
    auto round_lo = [&](uint64_t k) { return (uint64_t)(((unsigned __int128)count * k) / rounds); };
    const double share = (double)count / ((double)rounds * (double)n);   // units per replica per exchange
    std::vector<int64_t> bounds((size_t)n + 1);
    if (part && (rc = smore_source_parts(g->ctx[0], (int)n, bounds.data()))) return gfail(g, 0, rc);
    if (walkpart) {
        if ((rc = smore_walk_parts(g->ctx[0], (int)n, bounds.data()))) return gfail(g, 0, rc);
        for (size_t r = 0; r < n; ++r)
            if ((rc = smore_set_walk_owner(g->ctx[r], bounds[r], bounds[r + 1]))) return gfail(g, (int)r, rc);
    }
    const double c0v = g->c0 > 0 ? g->c0 : (part ? 2048.0 : 64.0);
    if (rule == SMORE_SYNC_ADAPTIVE) {
        const double updates = share * upu;
        const std::string key = scale_key(model, K, updates, c0v, (int)n, g->ctx[0]) + "/" + g->ctx[0]->census_key;
        bool same = true;
        for (smore_ctx* c : g->ctx) same = same && c->ex_scale_key == key;
        if (!same) {
            std::vector<float> sc[2];
            if ((rc = adaptive_scales(g->ctx[0], model, K, updates, c0v, (int)n, sc))) return gfail(g, 0, rc);
            for (size_t r = 0; r < n; ++r)
                if ((rc = upload_scales(g->ctx[r], sc, key))) return gfail(g, (int)r, rc);
        }
    }
    if (hot && (rc = ensure_hot(g, model, K, rows))) return rc;
    const int sub = hot ? g->launches : 1;
    for (uint64_t k = 0; k < rounds; ++k) {
        const uint64_t lo = round_lo(k), m = round_lo(k + 1) - lo;
        for (int j = 0; j < sub; ++j) {
            for (size_t r = 0; r < n; ++r) {
                // the walk partition: every replica runs the whole round (its pairs)
                const uint64_t b = walkpart ? lo : lo + (uint64_t)(((unsigned __int128)m * r) / n);
                const uint64_t e = walkpart ? lo + m : lo + (uint64_t)(((unsigned __int128)m * (r + 1)) / n);
                const uint64_t bj = b + (e - b) * (uint64_t)j / sub, ej = b + (e - b) * (uint64_t)(j + 1) / sub;
                if (ej > bj && (rc = run(g->ctx[r], begin + bj, begin + ej))) return gfail(g, (int)r, rc);
            }
            if (hot && (rc = group_hot_exchange(g))) return rc;
        }
        if ((rc = group_exchange_begin(g, rule))) return rc;
    }
    for (size_t r = 0; r < n; ++r)
        if ((rc = exchange_end(g->ctx[r]))) return gfail(g, (int)r, rc);
    if ((part || walkpart) && (rc = gather_sources(g, bounds))) return rc;
    if ((rc = group_sync(g))) return rc;
    for (size_t r = 0; walkpart && r < n; ++r)
        if ((rc = smore_set_walk_owner(g->ctx[r], 0, -1))) return gfail(g, (int)r, rc);
    return SMORE_OK;
}

// the block schedule applies: asked for (the default), more than one replica,
// and the C++ rules (the Go rules keep the replicas)
static bool blocks_for(const smore_group* g) {
    return g->schedule == SMORE_SCHED_BLOCKS && g->ctx.size() > 1 && g->ctx[0]->semantics == SMORE_SEM_CPP;
}

// the census key of a walk-model call: the model and every argument that
// changes which rows its records touch (walk law, window, K, seed)
static std::string census_key(const char* model, std::initializer_list<double> args) {
    std::string k = model;
    char b[40];
    for (double a : args) {
        snprintf(b, sizeof b, "/%.17g", a);
        k += b;
    }
    return k;
}

extern "C" {

// ---------------------------------------------------------------- one process, N GPUs
int smore_group_create(const int* devices, int n, smore_group** out) {
    if (!out || !devices || n < 1 || n > 64) return SMORE_EINVAL;
    *out = nullptr;
    // all replicas on one device (a repeated id): local collectives, no RCCL;
    // otherwise every device must be distinct (one RCCL rank per GPU)
    bool local = n > 1, distinct = true;
    for (int r = 1; r < n; ++r) local = local && devices[r] == devices[0];
    for (int r = 0; r < n; ++r)
        for (int q = 0; q < r; ++q) distinct = distinct && devices[q] != devices[r];
    if (n > 1 && !local && !distinct) return SMORE_EINVAL;
    smore_group* g = new smore_group();
    for (int r = 0; r < n; ++r) {
        smore_ctx* c = nullptr;
        const int rc = smore_create(devices[r], &c);
        if (rc) {
            smore_group_destroy(g);
            return rc;
        }
        g->ctx.push_back(c);
    }
    if (local) {
        g->local = true;
        g->lev.assign((size_t)n, nullptr);
        bool ok = hipSetDevice(devices[0]) == hipSuccess &&
                  hipEventCreateWithFlags(&g->ldone, hipEventDisableTiming) == hipSuccess;
        for (int r = 0; r < n && ok; ++r) ok = hipEventCreateWithFlags(&g->lev[r], hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            smore_group_destroy(g);
            return SMORE_EHIP;
        }
        for (int r = 0; r < n; ++r) {
            g->ctx[r]->comm = g;   // non-null: the exchange buffers are usable; never passed to RCCL
            g->ctx[r]->own_comm = false;
            g->ctx[r]->local_comm = true;
            g->ctx[r]->nranks = n;
            g->ctx[r]->rank = r;
        }
    } else if (n > 1) {
        Rccl* L = rccl();
        if (!L) {
            smore_group_destroy(g);
            return SMORE_EHIP;
        }
        g->comms.assign((size_t)n, nullptr);
        if (L->init_all(g->comms.data(), n, devices) != ncclSuccess) {
            g->comms.clear();
            smore_group_destroy(g);
            return SMORE_EHIP;
        }
        for (int r = 0; r < n; ++r) {
            g->ctx[r]->comm = g->comms[r];
            g->ctx[r]->own_comm = false;
            g->ctx[r]->nranks = n;
            g->ctx[r]->rank = r;
        }
    }
    *out = g;
    return SMORE_OK;
}

void smore_group_destroy(smore_group* g) {
    if (!g) return;
    for (smore_ctx* c : g->ctx) {
        smore_exchange_release(c);
        smore_destroy(c);
    }
    if (!g->comms.empty()) comm_release(rccl(), g->comms.data(), (int)g->comms.size());
    for (hipEvent_t e : g->lev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : g->bdone)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : g->brecv)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : g->hready)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : g->hdone)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : g->lser)
        if (e) (void)hipEventDestroy(e);
    if (g->ldone) (void)hipEventDestroy(g->ldone);
    delete g;
}

int smore_group_size(const smore_group* g) { return g ? (int)g->ctx.size() : 0; }

int smore_group_set_adaptive(smore_group* g, double c0) {
    if (!g || !(c0 > 0.0 || c0 == -1.0)) return SMORE_EINVAL;
    g->c0 = c0;
    return SMORE_OK;
}

int smore_group_set_partition(smore_group* g, int on) {
    if (!g) return SMORE_EINVAL;
    g->partition = on != 0;
    return SMORE_OK;
}

int smore_group_set_walk_partition(smore_group* g, int on) {
    if (!g) return SMORE_EINVAL;
    g->walk_partition = on != 0;
    return SMORE_OK;
}

int smore_group_set_schedule(smore_group* g, int schedule) {
    if (!g || (schedule != SMORE_SCHED_REPLICAS && schedule != SMORE_SCHED_BLOCKS)) return SMORE_EINVAL;
    g->schedule = schedule;
    return SMORE_OK;
}

int smore_group_set_hot_exchange(smore_group* g, int64_t rows, int launches) {
    if (!g || launches < 1) return SMORE_EINVAL;
    g->hot_rows = rows < 0 ? -1 : rows;
    g->launches = launches;
    return SMORE_OK;
}

smore_ctx* smore_group_ctx(smore_group* g, int rank) {
    if (!g || rank < 0 || rank >= (int)g->ctx.size()) return nullptr;
    return g->ctx[rank];
}

const char* smore_group_last_error(const smore_group* g) { return g ? g->err.c_str() : "null group"; }

int smore_group_load_edgelist(smore_group* g, const char* path, int undirected, int vm, int nm) {
    if (!g) return SMORE_EINVAL;
    int rc = smore_load_edgelist(g->ctx[0], path, undirected, vm, nm);
    if (rc) return gfail(g, 0, rc);
    return replicate_graph(g);
}

int smore_group_set_graph_edges(smore_group* g, int64_t V, int64_t E, const int32_t* src, const int32_t* dst,
                                const double* w, int vm, int nm) {
    if (!g) return SMORE_EINVAL;
    int rc = smore_set_graph_edges(g->ctx[0], V, E, src, dst, w, vm, nm);
    if (rc) return gfail(g, 0, rc);
    return replicate_graph(g);
}

int smore_group_set_semantics(smore_group* g, int semantics) {
    if (!g) return SMORE_EINVAL;
    for (size_t r = 0; r < g->ctx.size(); ++r) {
        // the host tables are shared: replica 0 rebuilds them, the builders are
        // idempotent, every replica uploads its own device copy
        int rc = smore_set_semantics(g->ctx[r], semantics);
        if (rc) return gfail(g, (int)r, rc);
    }
    return SMORE_OK;
}

int smore_group_set_alias(smore_group* g, int which, const double* prob, const int64_t* alias, int64_t n) {
    if (!g) return SMORE_EINVAL;
    for (size_t r = 0; r < g->ctx.size(); ++r) {
        int rc = smore_set_alias(g->ctx[r], which, prob, alias, n);
        if (rc) return gfail(g, (int)r, rc);
    }
    return SMORE_OK;
}

int smore_group_set_node_types(smore_group* g, const int32_t* node_type, int ntypes) {
    if (!g) return SMORE_EINVAL;
    for (size_t r = 0; r < g->ctx.size(); ++r) {
        int rc = smore_set_node_types(g->ctx[r], node_type, ntypes);
        if (rc) return gfail(g, (int)r, rc);
    }
    return SMORE_OK;
}

int smore_group_set_temporal_edges(smore_group* g, int64_t E, const int32_t* src, const int32_t* dst,
                                   const double* ts) {
    if (!g) return SMORE_EINVAL;
    for (size_t r = 0; r < g->ctx.size(); ++r) {
        int rc = smore_set_temporal_edges(g->ctx[r], E, src, dst, ts);
        if (rc) return gfail(g, (int)r, rc);
    }
    return SMORE_OK;
}

int smore_group_alloc_tables(smore_group* g, int dim, int ntables) {
    if (!g) return SMORE_EINVAL;
    if (ntables == 4 && !g->ctx.empty())   // CSE runs on one context
        return gfail(g, 0, fail(g->ctx[0], SMORE_ESTATE, "a group has no four-table (CSE) contexts"));
    for (size_t r = 0; r < g->ctx.size(); ++r) {
        int rc = smore_alloc_tables(g->ctx[r], dim, ntables);
        if (rc) return gfail(g, (int)r, rc);
    }
    return SMORE_OK;
}

int smore_group_broadcast_tables(smore_group* g) {
    if (!g) return SMORE_EINVAL;
    if (g->ctx.size() == 1) return SMORE_OK;
    int rc;
    for (size_t r = 0; r < g->ctx.size(); ++r) {
        smore_ctx* c = g->ctx[r];
        if (c->ntables < 1 || !c->d_table[0]) return gfail(g, (int)r, fail(c, SMORE_ESTATE, "tables not allocated"));
        if ((rc = smore_synchronize(c))) return gfail(g, (int)r, rc);
    }
    const size_t n = table_floats(g->ctx[0]);
    const std::vector<hipStream_t> st = compute_streams(g);
    for (int t = 0; t < g->ctx[0]->ntables; ++t) {
        std::vector<float*> buf;
        for (smore_ctx* c : g->ctx) buf.push_back(c->d_table[t]);
        if ((rc = coll_broadcast(g, buf, n, 0, st, "ncclBroadcast"))) return rc;
    }
    return group_sync(g);
}

int smore_group_train_edges(smore_group* g, int model, uint64_t begin, uint64_t count, uint64_t total, int K,
                            double alpha0, double reg, uint64_t seed, int mode, uint64_t sync_samples, int mean) {
    if (!g) return SMORE_EINVAL;
    if (g->ctx.size() == 1)
        return gfail(g, 0, smore_train_edges(g->ctx[0], model, begin, count, total, K, alpha0, reg, seed, mode));
    if (blocks_for(g) && model == SMORE_LINE2)
        return group_block_edges(g, begin, count, sync_samples, total, K, alpha0, seed, mode);
    return group_rounds(g, begin, begin + count, sync_samples, mean,
                        [&](smore_ctx* c, uint64_t b, uint64_t e) {
                            return smore_train_edges_async(c, model, b, e - b, total, K, alpha0, reg, seed, mode);
                        },
                        model, K, 1.0, model == SMORE_LINE2);
}

int smore_group_train_deepwalk(smore_group* g, uint64_t walk_begin, uint64_t walk_end, int walk_times,
                               int walk_steps, int window, int K, double alpha0, uint64_t seed, const int64_t* order,
                               int mode, uint64_t sync_walks, int mean) {
    if (!g) return SMORE_EINVAL;
    if (g->ctx.size() == 1)
        return gfail(g, 0, smore_train_deepwalk(g->ctx[0], walk_begin, walk_end, walk_times, walk_steps, window, K,
                                                alpha0, seed, order, mode));
    if (blocks_for(g))
        return group_block_walks(g, 0, walk_begin, walk_end, walk_times, walk_steps, window, 0, K, alpha0, seed, order,
                                 mode, sync_walks);
    return group_rounds(g, walk_begin, walk_end, sync_walks, mean,
                        [&](smore_ctx* c, uint64_t b, uint64_t e) {
                            return smore_train_deepwalk_async(c, b, e, walk_times, walk_steps, window, K, alpha0,
                                                              seed, order, mode);
                        },
                        SMORE_CENSUS, K, 1.0, false,
                        census_key("deepwalk", {(double)walk_times, (double)walk_steps, (double)window, (double)K, (double)seed}), true);
}

int smore_group_train_node2vec(smore_group* g, uint64_t walk_begin, uint64_t walk_end, int walk_times,
                               int walk_steps, int window, int K, double alpha0, double p, double q, uint64_t seed,
                               const int64_t* order, int mode, uint64_t sync_walks, int mean) {
    if (!g) return SMORE_EINVAL;
    if (g->ctx.size() == 1)
        return gfail(g, 0, smore_train_node2vec(g->ctx[0], walk_begin, walk_end, walk_times, walk_steps, window, K,
                                                alpha0, p, q, seed, order, mode));
    return group_rounds(g, walk_begin, walk_end, sync_walks, mean,
                        [&](smore_ctx* c, uint64_t b, uint64_t e) {
                            return smore_train_node2vec_async(c, b, e, walk_times, walk_steps, window, K, alpha0, p,
                                                              q, seed, order, mode);
                        },
                        SMORE_CENSUS, K, 1.0, false,
                        census_key("node2vec", {(double)walk_times, (double)walk_steps, (double)window, (double)K, p, q, (double)seed}), true);
}

int smore_group_train_metapath2vec(smore_group* g, uint64_t walk_begin, uint64_t walk_end, int walk_times,
                                   int walk_steps, int window, int K, double alpha0, const int32_t* paths,
                                   const int32_t* path_lens, int npaths, uint64_t seed, const int64_t* order,
                                   int mode, uint64_t sync_walks, int mean) {
    if (!g) return SMORE_EINVAL;
    if (g->ctx.size() == 1)
        return gfail(g, 0, smore_train_metapath2vec(g->ctx[0], walk_begin, walk_end, walk_times, walk_steps, window,
                                                    K, alpha0, paths, path_lens, npaths, seed, order, mode));
    return group_rounds(g, walk_begin, walk_end, sync_walks, mean,
                        [&](smore_ctx* c, uint64_t b, uint64_t e) {
                            return smore_train_metapath2vec_async(c, b, e, walk_times, walk_steps, window, K,
                                                                  alpha0, paths, path_lens, npaths, seed, order,
                                                                  mode);
                        },
                        SMORE_CENSUS, K, 1.0, false,
                        census_key("metapath2vec", {(double)walk_times, (double)walk_steps, (double)window, (double)K, (double)npaths, (double)seed}), true);
}

int smore_group_train_ctdne(smore_group* g, uint64_t walk_begin, uint64_t walk_end, int walk_times, int walk_steps,
                            int window, int K, double alpha0, double time_window, uint64_t seed,
                            const int64_t* order, int mode, uint64_t sync_walks, int mean) {
    if (!g) return SMORE_EINVAL;
    if (g->ctx.size() == 1)
        return gfail(g, 0, smore_train_ctdne(g->ctx[0], walk_begin, walk_end, walk_times, walk_steps, window, K,
                                             alpha0, time_window, seed, order, mode));
    return group_rounds(g, walk_begin, walk_end, sync_walks, mean,
                        [&](smore_ctx* c, uint64_t b, uint64_t e) {
                            return smore_train_ctdne_async(c, b, e, walk_times, walk_steps, window, K, alpha0,
                                                           time_window, seed, order, mode);
                        },
                        SMORE_CENSUS, K, 1.0, false,
                        census_key("ctdne", {(double)walk_times, (double)walk_steps, (double)window, (double)K, time_window, (double)seed}), true);
}

int smore_group_train_walklets(smore_group* g, uint64_t walk_begin, uint64_t walk_end, int walk_times, int walk_steps,
                               int window_min, int window_max, int K, double alpha0, uint64_t seed, int mode,
                               uint64_t sync_walks, int mean) {
    if (!g) return SMORE_EINVAL;
    if (g->ctx.size() == 1)
        return gfail(g, 0, smore_train_walklets(g->ctx[0], walk_begin, walk_end, walk_times, walk_steps, window_min,
                                                window_max, K, alpha0, seed, mode));
    if (blocks_for(g))
        return group_block_walks(g, 1, walk_begin, walk_end, walk_times, walk_steps, window_max, window_min, K, alpha0,
                                 seed, nullptr, mode, sync_walks);
    return group_rounds(g, walk_begin, walk_end, sync_walks, mean,
                        [&](smore_ctx* c, uint64_t b, uint64_t e) {
                            return smore_train_walklets_async(c, b, e, walk_times, walk_steps, window_min,
                                                              window_max, K, alpha0, seed, mode);
                        },
                        SMORE_CENSUS, K, 1.0, false,
                        census_key("walklets", {(double)walk_times, (double)walk_steps, (double)window_min, (double)window_max, (double)K, (double)seed}), true);
}

int smore_group_train_app(smore_group* g, uint64_t unit_begin, uint64_t unit_end, int walk_times, int sample_times,
                          double jump, int K, double alpha0, uint64_t seed, const int64_t* order, int mode,
                          uint64_t sync_units, int mean) {
    if (!g) return SMORE_EINVAL;
    if (g->ctx.size() == 1)
        return gfail(g, 0, smore_train_app(g->ctx[0], unit_begin, unit_end, walk_times, sample_times, jump, K, alpha0,
                                           seed, order, mode));
    return group_rounds(g, unit_begin, unit_end, sync_units, mean,
                        [&](smore_ctx* c, uint64_t b, uint64_t e) {
                            return smore_train_app_async(c, b, e, walk_times, sample_times, jump, K, alpha0, seed,
                                                         order, mode);
                        },
                        SMORE_CENSUS, K, 1.0, false,
                        census_key("app", {(double)walk_times, (double)sample_times, jump, (double)K, (double)seed}));
}

int smore_group_train_hpe(smore_group* g, uint64_t begin, uint64_t count, uint64_t total, int walk_steps, int K,
                          double reg, double alpha0, uint64_t seed, int mode, uint64_t sync_samples, int mean) {
    if (!g) return SMORE_EINVAL;
    if (g->ctx.size() == 1)
        return gfail(g, 0, smore_train_hpe(g->ctx[0], begin, count, total, walk_steps, K, reg, alpha0, seed, mode));
    return group_rounds(g, begin, begin + count, sync_samples, mean,
                        [&](smore_ctx* c, uint64_t b, uint64_t e) {
                            return smore_train_hpe_async(c, b, e - b, total, walk_steps, K, reg, alpha0, seed, mode);
                        },
                        SMORE_CENSUS, K, 1.0, false,
                        census_key("hpe", {(double)walk_steps, (double)K, (double)total, (double)seed}));
}

}  // extern "C"

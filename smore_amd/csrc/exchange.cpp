// exchange.cpp -- multi-GPU replicas over RCCL in the C ABI.
//
// The reference scales one training run over CPU threads sharing the tables
// (LINE::Train's `#pragma omp parallel for` over workers, src/model/LINE.cpp:162;
// Go goroutines, internal/models/line/line.go:96-146).  Here every GPU holds a
// replica of the graph and of the tables, trains a disjoint range of global
// sample indices, and the replicas exchange table deltas over RCCL (xGMI):
//
//   begin  (after a step, context stream):  D = T - S;  R = D;  S = T
//          all-reduce R (SUM) on the exchange stream, overlapping the next step
//   end    (before the next begin):         X = scale*R - D;  T += X;  S += X
//          (end fused with the next begin: delta_cycle, replica_sync.hip)
//
// so every sample's update lands on every replica one exchange late, and the
// next D is again only this replica's own updates.  Two ways to drive it:
//   * one process per GPU: smore_comm_unique_id / smore_comm_init, then
//     smore_exchange_reset / _begin / _end around the training calls;
//   * one process, N GPUs: smore_group_* (group.cpp; ncclCommInitAll, one host thread
//     enqueues every replica's work; the collectives of all replicas go out in
//     one ncclGroupStart/End).
// RCCL is loaded on first use (dlopen librccl.so.1): single-GPU users and the
// host-only context never load it.  A group whose replicas all sit on ONE
// device (smore_group_create with a repeated device id) runs the same rounds
// with its collectives as device passes on that GPU (local_sum_kernel, stream-
// ordered copies) and no RCCL: the multi-replica path on a one-GPU machine
// (tests, the replica-quality runs of DESIGN.md 10).
#include <dlfcn.h>

#include <mutex>

#include "group.h"
#include "hot_exchange.h"

using namespace smore_host;

namespace smore_host {

static double g_comm_timeout = -1.0;   // smore_set_comm_timeout; < 0: comm_timeout_default()

double comm_timeout() { return g_comm_timeout > 0 ? g_comm_timeout : comm_timeout_default(); }

// the RCCL table (comm_watch.h): loaded on first use
Rccl* rccl() {
    static Rccl r;
    static bool ok = false;
    static std::once_flag once;
    std::call_once(once, [] {
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) {
            r.err = std::string("cannot load RCCL: ") + dlerror();
            return;
        }
#define SMORE_SYM(field, name)                                          \
    r.field = reinterpret_cast<decltype(r.field)>(dlsym(h, #name));     \
    if (!r.field) {                                                     \
        r.err = "RCCL lacks " #name;                                    \
        return;                                                         \
    }
        SMORE_SYM(get_unique_id, ncclGetUniqueId)
        SMORE_SYM(init_rank, ncclCommInitRank)
        SMORE_SYM(init_all, ncclCommInitAll)
        SMORE_SYM(destroy, ncclCommDestroy)
        SMORE_SYM(abort, ncclCommAbort)
        SMORE_SYM(async_error, ncclCommGetAsyncError)
        SMORE_SYM(all_reduce, ncclAllReduce)
        SMORE_SYM(broadcast, ncclBroadcast)
        SMORE_SYM(send, ncclSend)
        SMORE_SYM(recv, ncclRecv)
        SMORE_SYM(group_start, ncclGroupStart)
        SMORE_SYM(group_end, ncclGroupEnd)
        SMORE_SYM(error_string, ncclGetErrorString)
#undef SMORE_SYM
        ok = true;
    });
    return ok ? &r : nullptr;
}

int nccl_fail(smore_ctx* c, const char* what, ncclResult_t r) {
    Rccl* L = rccl();
    return fail(c, SMORE_EHIP, std::string(what) + ": " + (L ? L->error_string(r) : "RCCL unavailable"));
}

#define NCCLCHK(c, what, expr)                                   \
    do {                                                         \
        ncclResult_t r_ = (expr);                                \
        if (r_ != ncclSuccess) return nccl_fail((c), what, r_);  \
    } while (0)

size_t table_floats(const smore_ctx* c) { return (size_t)c->g->V * (size_t)c->dpad; }

// exchange buffers S, D, R per table and the exchange stream / events
static int ensure_exchange(smore_ctx* c) {
    int rc;
    if ((rc = set_device(c))) return rc;
    if (!c->comm_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
    if (!c->ex_ready) HIPCHK(c, hipEventCreateWithFlags(&c->ex_ready, hipEventDisableTiming));
    if (!c->ex_done) HIPCHK(c, hipEventCreateWithFlags(&c->ex_done, hipEventDisableTiming));
    const size_t n = table_floats(c);
    if (c->ex_n == n && c->ex_tables == c->ntables) return SMORE_OK;
    for (auto& t : c->ex_buf)
        for (float*& p : t) dfree(p);
    c->ex_n = 0;
    c->ex_tables = 0;
    c->ex_pending = false;
    for (int t = 0; t < c->ntables; ++t)
        for (float*& p : c->ex_buf[t]) HIPCHK(c, hipMalloc((void**)&p, std::max<size_t>(n, 4) * sizeof(float)));
    c->ex_n = n;
    c->ex_tables = c->ntables;
    return SMORE_OK;
}

static int check_comm(smore_ctx* c) {
    if (!c) return SMORE_EINVAL;
    if (int rc_ = refuse_cse(c)) return rc_;
    if (!c->comm) return fail(c, SMORE_ESTATE, "no communicator (smore_comm_init / smore_group_create)");
    if (c->ntables < 1 || !c->d_table[0]) return fail(c, SMORE_ESTATE, "tables not allocated");
    return ensure_exchange(c);
}

// S = T for every table: the replicas start from identical tables
int exchange_reset(smore_ctx* c) {
    int rc;
    if ((rc = check_comm(c))) return rc;
    if (c->ex_pending) {
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ex_done, 0));
        c->ex_pending = false;
    }
    for (int t = c->ex_t0; t < c->ntables; ++t)
        HIPCHK(c, hipMemcpyAsync(c->ex_buf[t][0], c->d_table[t], c->ex_n * sizeof(float), hipMemcpyDeviceToDevice,
                                 c->stream));
    return SMORE_OK;
}

// the uniform scale of the summed deltas under the in-flight exchange's rule
static float rule_scale(const smore_ctx* c) { return c->ex_mode == SMORE_SYNC_MEAN ? 1.0f / (float)c->nranks : 1.0f; }

// the fused passes of an exchange's begin on the context stream (folding the
// in-flight exchange in first), then the hand-off event for the collective
int exchange_passes(smore_ctx* c, int mode) {
    int rc;
    if ((rc = set_device(c))) return rc;
    if (mode < SMORE_SYNC_SUM || mode > SMORE_SYNC_ADAPTIVE) return fail(c, SMORE_EINVAL, "bad exchange rule");
    if (mode == SMORE_SYNC_ADAPTIVE && !c->ex_scale[0])
        return fail(c, SMORE_ESTATE, "adaptive exchange without row scales (smore_exchange_set_adaptive)");
    if (c->ex_pending) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ex_done, 0));
    for (int t = c->ex_t0; t < c->ntables; ++t) {
        float* T = c->d_table[t];
        float* const* b = c->ex_buf[t];
        if (!c->ex_pending) HIPCHK(c, launch_delta_begin(T, b[0], b[1], b[2], c->ex_n, c->cus, c->stream));
        else if (c->ex_mode == SMORE_SYNC_ADAPTIVE)
            HIPCHK(c, launch_delta_cycle_rows(T, b[0], b[1], b[2], c->ex_scale[t], (uint64_t)c->g->V, c->dpad, c->cus,
                                              c->stream));
        else HIPCHK(c, launch_delta_cycle(T, b[0], b[1], b[2], rule_scale(c), c->ex_n, c->cus, c->stream));
    }
    HIPCHK(c, hipEventRecord(c->ex_ready, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->comm_stream, c->ex_ready, 0));
    c->ex_mode = mode;
    return SMORE_OK;
}

static int exchange_collective(smore_ctx* c) {
    Rccl* L = rccl();
    for (int t = c->ex_t0; t < c->ntables; ++t)
        NCCLCHK(c, "ncclAllReduce",
                L->all_reduce(c->ex_buf[t][2], c->ex_buf[t][2], c->ex_n, ncclFloat32, ncclSum, (ncclComm_t)c->comm,
                              c->comm_stream));
    c->coll_queued = true;
    return SMORE_OK;
}

int exchange_posted(smore_ctx* c) {
    int rc;
    if ((rc = set_device(c))) return rc;
    HIPCHK(c, hipEventRecord(c->ex_done, c->comm_stream));
    c->ex_pending = true;
    return SMORE_OK;
}

int exchange_end(smore_ctx* c) {
    int rc;
    if ((rc = check_comm(c))) return rc;
    if (!c->ex_pending) return SMORE_OK;
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ex_done, 0));
    for (int t = c->ex_t0; t < c->ntables; ++t) {
        float* const* b = c->ex_buf[t];
        if (c->ex_mode == SMORE_SYNC_ADAPTIVE)
            HIPCHK(c, launch_delta_end_rows(c->d_table[t], b[0], b[1], b[2], c->ex_scale[t], (uint64_t)c->g->V,
                                            c->dpad, c->cus, c->stream));
        else HIPCHK(c, launch_delta_end(c->d_table[t], b[0], b[1], b[2], rule_scale(c), c->ex_n, c->cus, c->stream));
    }
    c->ex_pending = false;
    return SMORE_OK;
}

// the adaptive rule's per-row scales (smore_hip.h SMORE_SYNC_ADAPTIVE) for
// `updates` samples of `model` per rank per exchange over `nranks` ranks, from
// the sampler marginals of c's graph
int adaptive_scales(smore_ctx* c, int model, int K, double updates, double c0, int nranks,
                    std::vector<float> (&out)[2]) {
    const int64_t V = c->g->V;
    std::vector<double> rate((size_t)V);
    for (int t = 0; t < c->ntables; ++t) {
        int rc;
        if ((rc = smore_row_rates(c, model, K, t, V, rate.data()))) return rc;
        out[t].resize((size_t)V);
        for (int64_t v = 0; v < V; ++v) {
            const double k = rate[v] * updates * nranks;
            const double sv = k > c0 ? c0 / k : 1.0;
            out[t][v] = (float)(sv + (1.0 - sv) / nranks);
        }
    }
    return SMORE_OK;
}

int upload_scales(smore_ctx* c, const std::vector<float> (&sc)[2], const std::string& key) {
    int rc;
    if ((rc = set_device(c))) return rc;
    // an in-flight exchange's end reads the old scales on the stream: replace
    // them only after it drained
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int t = 0; t < 2; ++t) {
        dfree(c->ex_scale[t]);
        if (t < c->ntables && (rc = upload(c, c->ex_scale[t], sc[t].data(), sc[t].size()))) return rc;
    }
    c->ex_scale_key = key;
    return SMORE_OK;
}

std::string scale_key(int model, int K, double updates, double c0, int nranks, const smore_ctx* c) {
    char key[160];
    snprintf(key, sizeof key, "%d/%d/%.17g/%.17g/%d/%lld/%d/%llu", model, K, updates, c0, nranks, (long long)c->g->V,
             c->ntables, model == SMORE_CENSUS ? (unsigned long long)c->census_gen : 0ull);
    return key;
}

}  // namespace smore_host

void smore_exchange_release(smore_ctx* c) {
    if (!c) return;
    if (c->device >= 0) (void)hipSetDevice(c->device);
    if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
    for (auto& t : c->ex_buf)
        for (float*& p : t) dfree(p);
    for (int t = 0; t < 2; ++t) {
        dfree(c->hot_idx[t]);
        dfree(c->hot_buf[t][0]);
        dfree(c->hot_buf[t][1]);
    }
    c->hot_n = 0;
    c->hot_ex_key.clear();
    for (float*& p : c->ex_scale) dfree(p);
    c->ex_scale_key.clear();
    if (c->comm && c->own_comm) {
        ncclComm_t cm = (ncclComm_t)c->comm;
        comm_release(rccl(), &cm, 1);
    }
    c->comm = nullptr;
    if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
    if (c->ex_ready) (void)hipEventDestroy(c->ex_ready);
    if (c->ex_done) (void)hipEventDestroy(c->ex_done);
    c->comm_stream = nullptr;
    c->ex_ready = c->ex_done = nullptr;
}

namespace smore_host {
// smore_synchronize of a context with its own communicator (one process per
// GPU): the stream's completion under the failure watch -- only when a
// collective was queued since the last watched sync (a long training call
// with no collective in flight is not a stuck peer)
int comm_sync(smore_ctx* c) {
    if (!c->comm || !c->own_comm || !c->coll_queued) return SMORE_OK;
    ncclComm_t cm = (ncclComm_t)c->comm;
    std::string why;
    auto ready = [&]() -> int {
        const hipError_t e = hipStreamQuery(c->stream);
        return e == hipSuccess ? 1 : e == hipErrorNotReady ? 0 : -1;
    };
    if (comm_watch(rccl(), &cm, 1, ready, comm_timeout(), why)) {
        c->comm = nullptr;   // aborted (freed): smore_exchange_release must not destroy it
        c->own_comm = false;
        return fail(c, SMORE_EHIP, why);
    }
    c->coll_queued = false;
    return SMORE_OK;
}
}  // namespace smore_host

extern "C" {

int smore_set_comm_timeout(double seconds) {
    if (!(seconds > 0.0) && seconds != -1.0) return SMORE_EINVAL;
    g_comm_timeout = seconds;
    return SMORE_OK;
}

int smore_comm_unique_id(unsigned char* id) {
    if (!id) return SMORE_EINVAL;
    Rccl* L = rccl();
    if (!L) return SMORE_EHIP;
    ncclUniqueId u;
    if (L->get_unique_id(&u) != ncclSuccess) return SMORE_EHIP;
    memcpy(id, u.internal, SMORE_COMM_ID_BYTES);
    return SMORE_OK;
}

int smore_comm_init(smore_ctx* c, int nranks, int rank, const unsigned char* id) {
    if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks) return SMORE_EINVAL;
    int rc;
    if ((rc = set_device(c))) return rc;
    Rccl* L = rccl();
    if (!L) return fail(c, SMORE_EHIP, "RCCL unavailable");
    if (c->comm) return fail(c, SMORE_ESTATE, "context already has a communicator");
    ncclUniqueId u;
    memcpy(u.internal, id, SMORE_COMM_ID_BYTES);
    ncclComm_t comm = nullptr;
    NCCLCHK(c, "ncclCommInitRank", L->init_rank(&comm, nranks, u, rank));
    c->comm = comm;
    c->own_comm = true;
    c->nranks = nranks;
    c->rank = rank;
    return SMORE_OK;
}

int smore_exchange_reset(smore_ctx* c) { return exchange_reset(c); }

int smore_exchange_begin(smore_ctx* c, int mean) {
    int rc;
    if ((rc = check_comm(c))) return rc;
    if (c->local_comm) return fail(c, SMORE_ESTATE, "a same-device group's replica: use the smore_group_* calls");
    if ((rc = exchange_passes(c, mean))) return rc;
    if ((rc = exchange_collective(c))) return rc;
    return exchange_posted(c);
}

int smore_exchange_end(smore_ctx* c) { return exchange_end(c); }

int smore_exchange_set_adaptive(smore_ctx* c, int model, int K, double updates, double c0) {
    if (!c || !(updates > 0.0) || !(c0 > 0.0)) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (c->ntables < 1) return fail(c, SMORE_ESTATE, "tables not allocated");
    if (int rc_ = refuse_cse(c)) return rc_;
    // the scales depend on the world size: only after smore_comm_init
    if (!c->comm) return fail(c, SMORE_ESTATE, "adaptive exchange before smore_comm_init");
    // an in-flight exchange's end applies the scales it was begun with
    if (c->ex_pending) return fail(c, SMORE_ESTATE, "adaptive scales changed while an exchange is in flight");
    const std::string key = scale_key(model, K, updates, c0, c->nranks, c);
    if (c->ex_scale_key == key) return SMORE_OK;
    std::vector<float> sc[2];
    int rc;
    if ((rc = adaptive_scales(c, model, K, updates, c0, c->nranks, sc))) return rc;
    return upload_scales(c, sc, key);
}

}  // extern "C"

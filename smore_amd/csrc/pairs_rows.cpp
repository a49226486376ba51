// pairs_rows.cpp -- caller pairs on caller-held rows: the rows a batch of
// pairs touches, row transfers to and from the tables, and the combining
// queue of concurrent callers (the Go UpdatePairs hook).
#include "train_host.h"

#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <vector>

using namespace smore_host;

extern "C" {

// The Philox spec on the host (device_common.h philox_block):
// the negatives smore_train_pairs will draw, without a device round trip.
static uint32_t philox_word(uint64_t seed, uint32_t stream, uint64_t unit, uint32_t slot) {
    uint32_t c0 = (uint32_t)unit, c1 = (uint32_t)(unit >> 32), c2 = slot >> 2, c3 = stream;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
    }
    const uint32_t w[4] = {c0, c1, c2, c3};
    return w[slot & 3];
}

int smore_pairs_rows(smore_ctx* c, const int32_t* v, const int32_t* cc, int64_t n, int K, uint64_t seed,
                     uint64_t unit, int32_t* w_ids, int64_t* nw, int32_t* c_ids, int64_t* nc) {
    if (!c || !nw || !nc || (n > 0 && (!v || !cc || !w_ids || !c_ids)) || n < 0 || K < 0 || K > 10)
        return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    const HostGraph& g = *c->g;
    const int64_t V = g.V;
    std::vector<int32_t> ws, cs;
    ws.reserve((size_t)n);
    cs.reserve((size_t)n * (K + 1));
    for (int64_t i = 0; i < n; ++i) {
        if (v[i] < 0 || v[i] >= V || cc[i] < 0 || cc[i] >= V) return fail(c, SMORE_EINVAL, "pair id out of range");
        ws.push_back(v[i]);
        cs.push_back(cc[i]);
        // caller_pair_kernel's draws: stream 3, unit + i / PAIR_BLOCK, slots
        // 2K (i % PAIR_BLOCK) + 2q (index), + 1 (p)
        const uint64_t u = unit + (uint64_t)i / PAIR_BLOCK;
        const uint32_t base = 2u * (uint32_t)K * (uint32_t)((uint64_t)i % PAIR_BLOCK);
        for (int q = 0; q < K; ++q) {
            const uint32_t ki = philox_word(seed, 3, u, base + 2u * (uint32_t)q);
            const uint32_t kp = philox_word(seed, 3, u, base + 2u * (uint32_t)q + 1u);
            const uint32_t ni = (uint32_t)(((uint64_t)ki * (uint64_t)V) >> 32);
            const AliasEntry e = g.ntab[ni];
            cs.push_back(kp < e.thresh ? (int32_t)ni : (e.alias & ID_MASK));
        }
    }
    std::sort(ws.begin(), ws.end());
    ws.erase(std::unique(ws.begin(), ws.end()), ws.end());
    std::sort(cs.begin(), cs.end());
    cs.erase(std::unique(cs.begin(), cs.end()), cs.end());
    std::copy(ws.begin(), ws.end(), w_ids);
    std::copy(cs.begin(), cs.end(), c_ids);
    *nw = (int64_t)ws.size();
    *nc = (int64_t)cs.size();
    return SMORE_OK;
}

// rows `ids` of table `which` from (to_table) / to a host buffer, through the
// device buffers of slot `which`, queued on the context stream (the host
// buffer is read / written when the stream gets there: synchronize first)
static int rows_io_async(smore_ctx* c, int which, const int32_t* ids, int64_t n, float* rows, bool to_table) {
    if (!c || n < 0 || (n > 0 && (!ids || !rows))) return SMORE_EINVAL;
    int rc;
    if ((rc = check_table(c, which))) return rc;
    if (n == 0) return SMORE_OK;
    const int slot = which & 1;   // a four-table context's tables 2, 3 share the two buffer slots
    for (int64_t i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= c->g->V) return fail(c, SMORE_EINVAL, "row id out of range");
    if ((rc = set_device(c))) return rc;
    if (c->io_cap[slot] < (size_t)n) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        dfree(c->d_io_ids[slot]);
        dfree(c->d_io_rows[slot]);
        c->io_cap[slot] = 0;
        const size_t cap = std::max<size_t>((size_t)n, 4096);
        HIPCHK(c, hipMalloc((void**)&c->d_io_ids[slot], cap * sizeof(int32_t)));
        HIPCHK(c, hipMalloc((void**)&c->d_io_rows[slot], cap * c->dim * sizeof(float)));
        c->io_cap[slot] = cap;
    }
    const size_t bytes = (size_t)n * c->dim * sizeof(float);
    HIPCHK(c, hipMemcpyAsync(c->d_io_ids[slot], ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (to_table) HIPCHK(c, hipMemcpyAsync(c->d_io_rows[slot], rows, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_rows_io(c->d_table[which], c->d_io_ids[slot], (uint64_t)n, c->dpad, c->dim, c->d_io_rows[slot],
                             to_table ? 1 : 0, c->stream));
    if (!to_table) HIPCHK(c, hipMemcpyAsync(rows, c->d_io_rows[slot], bytes, hipMemcpyDeviceToHost, c->stream));
    return SMORE_OK;
}

int smore_set_rows(smore_ctx* c, int which, const int32_t* ids, int64_t n, const float* rows) {
    int rc = rows_io_async(c, which, ids, n, const_cast<float*>(rows), true);
    if (rc == SMORE_OK && c && n > 0) HIPCHK(c, hipStreamSynchronize(c->stream));
    return rc;
}

int smore_get_rows(smore_ctx* c, int which, const int32_t* ids, int64_t n, float* rows) {
    int rc = rows_io_async(c, which, ids, n, rows, false);
    if (rc == SMORE_OK && c && n > 0) HIPCHK(c, hipStreamSynchronize(c->stream));
    return rc;
}

int smore_train_pairs_rows(smore_ctx* c, const int32_t* v, const int32_t* cc, int64_t n, int K, double alpha,
                           uint64_t seed, uint64_t unit, int mode, const int32_t* w_ids, int64_t nw, float* w_rows,
                           const int32_t* c_ids, int64_t nc, float* c_rows) {
    int rc;
    if (!c) return SMORE_EINVAL;
    if ((rc = rows_io_async(c, 0, w_ids, nw, w_rows, true))) return rc;
    if ((rc = rows_io_async(c, 1, c_ids, nc, c_rows, true))) return rc;
    if ((rc = train_pairs_core(c, v, cc, n, K, alpha, seed, unit, mode))) return rc;
    if ((rc = rows_io_async(c, 0, w_ids, nw, w_rows, false))) return rc;
    return sync_after(c, rows_io_async(c, 1, c_ids, nc, c_rows, false), true);
}

// ---------------------------------------------------------------- combining
// The reference's callers run UpdatePairs from `workers` goroutines at once,
// each on its own walk's ~380 pairs (internal/models/deepwalk/deepwalk.go:
// 96-120; pkg/pronet/optimizer.go:8-18).  A GPU call per batch costs a
// synchronisation and two small transfers whatever the batch, so a serialised
// hook loses to the CPU path once two goroutines run.  Flat combining: every
// caller copies its batch (pairs, row ids, rows) into a pinned staging slot of
// its own -- in parallel with the other callers -- and queues it; whichever
// finds the context idle becomes the leader, takes every request queued so far
// and runs them as ONE device call: per request in queue order, its rows up
// (asynchronous from pinned memory; rows an earlier request of the call
// already brought are NOT uploaded again, so each batch sees the rows the
// earlier ones wrote -- the serial order of the queue), its pairs, its rows
// back; one synchronisation; then every caller copies its rows out of its
// slot, again in parallel.  A request's rows come back as they are after its
// own batch.
struct PairSlot {   // pinned staging of one request; capacities in elements
    float *w_rows = nullptr, *c_rows = nullptr;
    int32_t *w_ids = nullptr, *c_ids = nullptr, *v = nullptr, *cc = nullptr, *w_sel = nullptr, *c_sel = nullptr;
    size_t cap[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

struct PairReq {
    int64_t n;
    int K;
    double alpha;
    uint64_t seed, unit;
    int mode;
    int64_t nw, nc;
    PairSlot* slot;
    int64_t msel_w = 0, msel_c = 0;   // rows this request uploads (not already on the device in this call)
    int rc = SMORE_OK;
    bool done = false;
};

struct PairCombiner {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<PairReq*> q;
    bool busy = false;
    uint64_t calls = 0, requests = 0;   // combined device calls, requests served
    std::mutex pool_mu;                 // the free slots
    std::vector<PairSlot*> pool;
    std::vector<PairSlot*> all;
    std::vector<uint8_t> seen[2];       // the leader's marks of the rows already brought (cleared after use)
    bool seen_dirty = false;            // a call failed before clearing its marks
    // device staging of one combined call
    float* d_rows = nullptr;
    int32_t *d_ids = nullptr, *d_sel = nullptr;
    size_t rows_cap = 0;   // rows
    ~PairCombiner() {
        for (PairSlot* p : all) {
            for (void* x : {(void*)p->w_rows, (void*)p->c_rows, (void*)p->w_ids, (void*)p->c_ids, (void*)p->v,
                            (void*)p->cc, (void*)p->w_sel, (void*)p->c_sel})
                if (x) (void)hipHostFree(x);
            delete p;
        }
        if (d_rows) (void)hipFree(d_rows);
        if (d_ids) (void)hipFree(d_ids);
        if (d_sel) (void)hipFree(d_sel);
    }
};

namespace {
// a pinned host buffer of at least `need` elements of `size` bytes
bool host_grow(void** p, size_t& cap, size_t need, size_t size) {
    if (need <= cap && *p) return true;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr;
    cap = 0;
    const size_t n = std::max<size_t>(need, 1024);
    if (hipHostMalloc(p, n * size, hipHostMallocDefault) != hipSuccess) return false;
    cap = n;
    return true;
}

PairSlot* slot_acquire(PairCombiner& pc, int64_t n, int64_t nw, int64_t nc, int dim) {
    PairSlot* s = nullptr;
    {
        std::lock_guard<std::mutex> g(pc.pool_mu);
        if (!pc.pool.empty()) {
            s = pc.pool.back();
            pc.pool.pop_back();
        } else {
            s = new PairSlot();
            pc.all.push_back(s);
        }
    }
    const size_t need[8] = {(size_t)nw * dim, (size_t)nc * dim, (size_t)nw, (size_t)nc, (size_t)n, (size_t)n,
                            (size_t)nw, (size_t)nc};
    void** buf[8] = {(void**)&s->w_rows, (void**)&s->c_rows, (void**)&s->w_ids, (void**)&s->c_ids, (void**)&s->v,
                     (void**)&s->cc, (void**)&s->w_sel, (void**)&s->c_sel};
    bool ok = true;
    for (int k = 0; k < 8 && ok; ++k) ok = host_grow(buf[k], s->cap[k], need[k], k < 2 ? sizeof(float) : sizeof(int32_t));
    if (!ok) {
        std::lock_guard<std::mutex> g(pc.pool_mu);
        pc.pool.push_back(s);
        return nullptr;
    }
    return s;
}

void slot_release(PairCombiner& pc, PairSlot* s) {
    std::lock_guard<std::mutex> g(pc.pool_mu);
    pc.pool.push_back(s);
}

// the leader: every request of the call, in queue order, on the stream
int combined_call(smore_ctx* c, PairCombiner& pc, const std::vector<PairReq*>& reqs) {
    const int dim = c->dim;
    size_t rows = 0;
    for (const PairReq* q : reqs) rows += (size_t)(q->nw + q->nc);
    if (pc.rows_cap < rows) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (pc.d_rows) (void)hipFree(pc.d_rows);
        if (pc.d_ids) (void)hipFree(pc.d_ids);
        if (pc.d_sel) (void)hipFree(pc.d_sel);
        pc.d_rows = nullptr;
        pc.d_ids = pc.d_sel = nullptr;
        pc.rows_cap = 0;
        const size_t cap = std::max<size_t>(rows * 2, 1 << 16);
        HIPCHK(c, hipMalloc((void**)&pc.d_rows, cap * dim * sizeof(float)));
        HIPCHK(c, hipMalloc((void**)&pc.d_ids, cap * sizeof(int32_t)));
        HIPCHK(c, hipMalloc((void**)&pc.d_sel, cap * sizeof(int32_t)));
        pc.rows_cap = cap;
    }
    // the rows each request must bring: those no earlier request of the call brought
    auto& seen = pc.seen;
    const int64_t V = c->g->V;
    for (auto& x : seen)
        if ((int64_t)x.size() != V || pc.seen_dirty) x.assign((size_t)V, 0);
    pc.seen_dirty = true;
    for (PairReq* q : reqs) {
        PairSlot* s = q->slot;
        q->msel_w = q->msel_c = 0;
        for (int64_t i = 0; i < q->nw; ++i)
            if (!seen[0][s->w_ids[i]]) {
                seen[0][s->w_ids[i]] = 1;
                s->w_sel[q->msel_w++] = (int32_t)i;
            }
        for (int64_t i = 0; i < q->nc; ++i)
            if (!seen[1][s->c_ids[i]]) {
                seen[1][s->c_ids[i]] = 1;
                s->c_sel[q->msel_c++] = (int32_t)i;
            }
    }
    int rc;
    size_t off = 0;
    for (PairReq* q : reqs) {
        PairSlot* s = q->slot;
        for (int t = 0; t < 2; ++t) {
            const int64_t n = t ? q->nc : q->nw, m = t ? q->msel_c : q->msel_w;
            if (n == 0) continue;
            float* dr = pc.d_rows + (off + (t ? (size_t)q->nw : 0)) * dim;
            int32_t* di = pc.d_ids + off + (t ? (size_t)q->nw : 0);
            int32_t* ds = pc.d_sel + off + (t ? (size_t)q->nw : 0);
            HIPCHK(c, hipMemcpyAsync(di, t ? s->c_ids : s->w_ids, n * sizeof(int32_t), hipMemcpyHostToDevice,
                                     c->stream));
            if (m > 0) {
                HIPCHK(c, hipMemcpyAsync(ds, t ? s->c_sel : s->w_sel, m * sizeof(int32_t), hipMemcpyHostToDevice,
                                         c->stream));
                HIPCHK(c, hipMemcpyAsync(dr, t ? s->c_rows : s->w_rows, (size_t)n * dim * sizeof(float),
                                         hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, launch_rows_put_sel(c->d_table[t], di, ds, (uint64_t)m, c->dpad, dim, dr, c->stream));
            }
        }
        q->rc = train_pairs_core(c, s->v, s->cc, q->n, q->K, q->alpha, q->seed, q->unit, q->mode);
        if (q->rc) return q->rc;
        for (int t = 0; t < 2; ++t) {
            const int64_t n = t ? q->nc : q->nw;
            if (n == 0) continue;
            float* dr = pc.d_rows + (off + (t ? (size_t)q->nw : 0)) * dim;
            int32_t* di = pc.d_ids + off + (t ? (size_t)q->nw : 0);
            HIPCHK(c, launch_rows_io(c->d_table[t], di, (uint64_t)n, c->dpad, dim, dr, 0, c->stream));
            HIPCHK(c, hipMemcpyAsync(t ? s->c_rows : s->w_rows, dr, (size_t)n * dim * sizeof(float),
                                     hipMemcpyDeviceToHost, c->stream));
        }
        off += (size_t)(q->nw + q->nc);
    }
    for (PairReq* q : reqs) {   // clear the marks this call set
        for (int64_t i = 0; i < q->msel_w; ++i) seen[0][q->slot->w_ids[q->slot->w_sel[i]]] = 0;
        for (int64_t i = 0; i < q->msel_c; ++i) seen[1][q->slot->c_ids[q->slot->c_sel[i]]] = 0;
    }
    pc.seen_dirty = false;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)rc;
    return SMORE_OK;
}
}  // namespace

int smore_train_pairs_rows_mt(smore_ctx* c, const int32_t* v, const int32_t* cc, int64_t n, int K, double alpha,
                              uint64_t seed, uint64_t unit, int mode, const int32_t* w_ids, int64_t nw, float* w_rows,
                              const int32_t* c_ids, int64_t nc, float* c_rows) {
    if (!c) return SMORE_EINVAL;
    if (n < 0 || nw < 0 || nc < 0 || (n > 0 && (!v || !cc)) || (nw > 0 && (!w_ids || !w_rows)) ||
        (nc > 0 && (!c_ids || !c_rows)))
        return SMORE_EINVAL;
    if (!c->has_graph || c->ntables < 2 || c->dim <= 0) return fail(c, SMORE_ESTATE, "pairs: no graph or tables");
    if (int rc_ = refuse_cse(c)) return rc_;
    const int64_t V = c->g->V;
    for (int64_t i = 0; i < nw; ++i)
        if (w_ids[i] < 0 || w_ids[i] >= V) return fail(c, SMORE_EINVAL, "row id out of range");
    for (int64_t i = 0; i < nc; ++i)
        if (c_ids[i] < 0 || c_ids[i] >= V) return fail(c, SMORE_EINVAL, "row id out of range");
    std::shared_ptr<PairCombiner> pc;
    {
        static std::mutex create_mu;   // the context's combiner, made once
        std::lock_guard<std::mutex> g(create_mu);
        if (!c->pair_comb) c->pair_comb = std::make_shared<PairCombiner>();
        pc = c->pair_comb;
    }
    const int dim = c->dim;
    PairSlot* slot = slot_acquire(*pc, n, nw, nc, dim);
    if (!slot) return fail(c, SMORE_EHIP, "pairs: pinned staging");
    // this caller's copies into its slot (in parallel with the other callers)
    std::copy(v, v + n, slot->v);
    std::copy(cc, cc + n, slot->cc);
    std::copy(w_ids, w_ids + nw, slot->w_ids);
    std::copy(c_ids, c_ids + nc, slot->c_ids);
    std::copy(w_rows, w_rows + (size_t)nw * dim, slot->w_rows);
    std::copy(c_rows, c_rows + (size_t)nc * dim, slot->c_rows);
    PairReq me{n, K, alpha, seed, unit, mode, nw, nc, slot};
    std::unique_lock<std::mutex> lk(pc->mu);
    pc->q.push_back(&me);
    pc->cv.wait(lk, [&] { return me.done || !pc->busy; });
    if (!me.done) {
        // leader: every queued request (its own among them) in one device call
        pc->busy = true;
        std::vector<PairReq*> reqs;
        reqs.swap(pc->q);
        lk.unlock();
        const int rc = set_device(c) ? SMORE_EHIP : combined_call(c, *pc, reqs);
        lk.lock();
        for (PairReq* q : reqs) {
            if (rc && !q->rc) q->rc = rc;
            q->done = true;
        }
        pc->calls++;
        pc->requests += reqs.size();
        pc->busy = false;
        lk.unlock();
        pc->cv.notify_all();
    } else {
        lk.unlock();
    }
    if (me.rc == SMORE_OK) {   // this caller's rows out of its slot (in parallel)
        std::copy(slot->w_rows, slot->w_rows + (size_t)nw * dim, w_rows);
        std::copy(slot->c_rows, slot->c_rows + (size_t)nc * dim, c_rows);
    }
    slot_release(*pc, slot);
    return me.rc;
}

int smore_pairs_combine_stats(const smore_ctx* c, uint64_t* calls, uint64_t* requests) {
    if (!c) return SMORE_EINVAL;
    std::shared_ptr<PairCombiner> pc = c->pair_comb;
    if (calls) *calls = pc ? pc->calls : 0;
    if (requests) *requests = pc ? pc->requests : 0;
    return SMORE_OK;
}

}  // extern "C"

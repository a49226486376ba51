// group_blocks.cpp -- the group side of the 2-D block schedule (blocks.cpp
// holds one replica's): the rotation of the C blocks between
// the replicas, the hub slots' exchange, and the two drivers that run a group
// call cell by cell.
#include <initializer_list>

#include "group.h"
#include "hot_exchange.h"

using namespace smore_host;

namespace {

// ---- the 2-D block schedule's group side (blocks.cpp holds one replica's):
// sub-round s trains cell (r, (2r + s) mod nb) on replica r; after it replica
// r sends that C block to r - 1, which trains it at sub-round s + 2, and
// receives the block r + 1 just trained.  Replica r's stream waits for the
// receive of the rotation two sub-rounds back before its sub-round, so a
// transfer overlaps one whole sub-round.  No row is replicated while it
// trains: nothing is all-reduced.
int ensure_block_events(smore_group* g) {
    const size_t n = g->ctx.size();
    if (g->bdone.size() == n) return SMORE_OK;
    g->bdone.assign(n, nullptr);
    g->brecv.assign(2 * n, nullptr);
    for (size_t r = 0; r < n; ++r) {
        smore_ctx* c = g->ctx[r];
        int rc;
        if ((rc = set_device(c))) return gfail(g, (int)r, rc);
        if (!c->comm_stream && hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking) != hipSuccess)
            return gfail(g, (int)r, fail(c, SMORE_EHIP, "block schedule: comm stream"));
        for (hipEvent_t* e : {&g->bdone[r], &g->brecv[2 * r], &g->brecv[2 * r + 1]})
            if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess)
                return gfail(g, (int)r, fail(c, SMORE_EHIP, "block schedule: events"));
    }
    return SMORE_OK;
}

float* block_rows(smore_ctx* c, int b) { return c->d_table[1] + (size_t)c->blk.cb[b] * c->dpad; }
size_t block_floats(const smore_ctx* c, int b) { return (size_t)(c->blk.cb[b + 1] - c->blk.cb[b]) * c->dpad; }

int group_rotate(smore_group* g, uint64_t s) {
    const size_t n = g->ctx.size();
    const int nb = 2 * (int)n;
    for (size_t r = 0; r < n; ++r) {
        smore_ctx* c = g->ctx[r];
        (void)hipSetDevice(c->device);
        if (hipEventRecord(g->bdone[r], c->stream) != hipSuccess)
            return gfail(g, (int)r, fail(c, SMORE_EHIP, "block rotation: event"));
    }
    if (g->local) {
        for (size_t r = 0; r < n; ++r) {
            smore_ctx *c = g->ctx[r], *d = g->ctx[(r + n - 1) % n];
            const int b = (int)((2 * r + s) % (uint64_t)nb);
            hipEvent_t done = g->brecv[2 * ((r + n - 1) % n) + (s & 1)];
            if (hipStreamWaitEvent(d->comm_stream, g->bdone[r], 0) != hipSuccess ||
                hipMemcpyAsync(block_rows(d, b), block_rows(c, b), block_floats(c, b) * sizeof(float),
                               hipMemcpyDeviceToDevice, d->comm_stream) != hipSuccess ||
                hipEventRecord(done, d->comm_stream) != hipSuccess)
                return gfail(g, (int)r, fail(c, SMORE_EHIP, "block rotation: local copy"));
        }
        return SMORE_OK;
    }
    Rccl* L = rccl();
    for (size_t r = 0; r < n; ++r) {
        (void)hipSetDevice(g->ctx[r]->device);
        if (hipStreamWaitEvent(g->ctx[r]->comm_stream, g->bdone[r], 0) != hipSuccess)
            return gfail(g, (int)r, fail(g->ctx[r], SMORE_EHIP, "block rotation: wait"));
    }
    ncclResult_t nr = L->group_start();
    for (size_t r = 0; r < n && nr == ncclSuccess; ++r) {
        smore_ctx* c = g->ctx[r];
        (void)hipSetDevice(c->device);
        const int b = (int)((2 * r + s) % (uint64_t)nb), b2 = (b + 2) % nb;
        nr = L->send(block_rows(c, b), block_floats(c, b), ncclFloat32, (int)((r + n - 1) % n), (ncclComm_t)c->comm,
                     c->comm_stream);
        if (nr == ncclSuccess)
            nr = L->recv(block_rows(c, b2), block_floats(c, b2), ncclFloat32, (int)((r + 1) % n), (ncclComm_t)c->comm,
                         c->comm_stream);
    }
    ncclResult_t ne = L->group_end();
    if (nr == ncclSuccess) nr = ne;
    if (nr != ncclSuccess) return gfail(g, 0, nccl_fail(g->ctx[0], "block rotation ncclSend/ncclRecv", nr));
    for (size_t r = 0; r < n; ++r) {
        (void)hipSetDevice(g->ctx[r]->device);
        if (hipEventRecord(g->brecv[2 * r + (s & 1)], g->ctx[r]->comm_stream) != hipSuccess)
            return gfail(g, (int)r, fail(g->ctx[r], SMORE_EHIP, "block rotation: event"));
    }
    return SMORE_OK;
}

// replica r's stream waits for the block it trains at sub-round s
int block_wait(smore_group* g, size_t r, uint64_t s) {
    if (s < 2) return SMORE_OK;
    smore_ctx* c = g->ctx[r];
    (void)hipSetDevice(c->device);
    if (hipStreamWaitEvent(c->stream, g->brecv[2 * r + (s & 1)], 0) != hipSuccess)
        return gfail(g, (int)r, fail(c, SMORE_EHIP, "block schedule: wait"));
    return SMORE_OK;
}

int hub_ex_finish(smore_group* g);

// after the last rotation: every transfer done before the tables are read;
// then every replica gets the W parts from their owners and the C blocks from
// their holders (after S sub-rounds block b sits on replica ((b - S) mod nb) / 2)
int block_finish(smore_group* g, uint64_t S) {
    const size_t n = g->ctx.size();
    const int nb = 2 * (int)n;
    int rc;
    for (size_t r = 0; r < n; ++r) {
        smore_ctx* c = g->ctx[r];
        (void)hipSetDevice(c->device);
        for (size_t q = 0; q < n; ++q) {
            if (!g->local && q != r) continue;   // RCCL: own transfers (send and receive) on own comm stream
            if (hipStreamWaitEvent(c->stream, g->brecv[2 * q], 0) != hipSuccess ||
                hipStreamWaitEvent(c->stream, g->brecv[2 * q + 1], 0) != hipSuccess)
                return gfail(g, (int)r, fail(c, SMORE_EHIP, "block schedule: drain"));
        }
    }
    // the hub slots back into their rows only now: the last rotation's
    // transfer carries the block's stale copy of those rows and would
    // overwrite a store queued ahead of the drain
    if ((rc = hub_ex_finish(g))) return rc;
    const std::vector<hipStream_t> st = compute_streams(g);
    smore_ctx* c0 = g->ctx[0];
    for (size_t p = 0; p < n; ++p) {
        std::vector<float*> rows;
        for (smore_ctx* c : g->ctx) rows.push_back(c->d_table[0] + (size_t)c0->blk.wb[p] * c->dpad);
        if ((rc = coll_broadcast(g, rows, (size_t)(c0->blk.wb[p + 1] - c0->blk.wb[p]) * c0->dpad, (int)p, st,
                                 "W parts ncclBroadcast")))
            return rc;
    }
    for (int b = 0; b < nb; ++b) {
        const int holder = (int)(((uint64_t)b + (uint64_t)nb - S % (uint64_t)nb) % (uint64_t)nb) / 2;
        std::vector<float*> rows;
        for (smore_ctx* c : g->ctx) rows.push_back(block_rows(c, b));
        if ((rc = coll_broadcast(g, rows, block_floats(c0, b), holder, st, "C blocks ncclBroadcast"))) return rc;
    }
    return group_sync(g);
}

// ---- the hub slots of the LINE-2 block schedule (blocks.cpp): every part
// trains its own copy of the H hub C rows in every cell; after each
// sub-round the copies' deltas are all-reduced one late (begin / cycle / end
// of replica_sync.hip on the slot rows, per-slot adaptive scales), on the
// comm streams ahead of the rotation
// the slots' adaptive rule's c0: LINE-2 2048 (the source-partitioned replica
// exchange's); walk models 64 (theirs: a C5 run is ~2000 pair updates per
// row in all, so a hub's copies are averaged sooner -- c0 2048 cost 1.11x
// one GPU's held-out loss at 8 parts, 64 1.026x)
double hub_c0(const smore_group* g) {
    const char* e = getenv("SMORE_HUB_C0");
    const double v = e ? atof(e) : 0.0;
    if (v > 0) return v;
    return g->ctx[0]->blk.model == SMORE_CENSUS ? 64.0 : 2048.0;
}

float* hub_slots(smore_ctx* c) { return c->d_table[1] + (size_t)c->g->V * c->dpad; }

int hub_ex_start(smore_group* g, double samples_per_exchange) {
    const size_t n = g->ctx.size();
    if (!g->ctx[0]->blk.H) return SMORE_OK;
    if (g->hready.size() != n) {
        g->hready.assign(n, nullptr);
        g->hdone.assign(n, nullptr);
        for (size_t r = 0; r < n; ++r) {
            (void)hipSetDevice(g->ctx[r]->device);
            if (hipEventCreateWithFlags(&g->hready[r], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&g->hdone[r], hipEventDisableTiming) != hipSuccess)
                return gfail(g, (int)r, fail(g->ctx[r], SMORE_EHIP, "hub exchange: events"));
        }
    }
    const double c0 = hub_c0(g);
    char key[96];
    snprintf(key, sizeof key, "%.17g/%.17g", samples_per_exchange, c0);
    for (size_t r = 0; r < n; ++r) {
        smore_ctx* c = g->ctx[r];
        auto& B = c->blk;
        int rc;
        if ((rc = set_device(c))) return gfail(g, (int)r, rc);
        const size_t nf = (size_t)B.H * c->dpad;
        for (float*& p : B.d_hub_ex)
            if (!p && hipMalloc((void**)&p, nf * sizeof(float)) != hipSuccess)
                return gfail(g, (int)r, fail(c, SMORE_EHIP, "hub exchange buffers"));
        if (B.hub_scale_key != key) {
            std::vector<float> sc((size_t)B.H);
            hub_scales(B, samples_per_exchange, c0, sc.data());
            if ((rc = upload(c, B.d_hub_scale, sc.data(), sc.size()))) return gfail(g, (int)r, rc);
            B.hub_scale_key = key;
        }
        if ((rc = smore_block_hubs_load(c))) return gfail(g, (int)r, rc);
        if (hipMemcpyAsync(B.d_hub_ex[0], hub_slots(c), nf * sizeof(float), hipMemcpyDeviceToDevice, c->stream) !=
            hipSuccess)
            return gfail(g, (int)r, fail(c, SMORE_EHIP, "hub exchange: snapshot"));
        B.hub_pending = false;
    }
    return SMORE_OK;
}

// after every replica's cell of a sub-round: the exchange pass on the compute
// stream, then the all-reduce of the slots' deltas on the comm streams
int hub_ex_post(smore_group* g) {
    const size_t n = g->ctx.size();
    if (!g->ctx[0]->blk.H) return SMORE_OK;
    std::vector<float*> bufs;
    std::vector<hipStream_t> st;
    for (size_t r = 0; r < n; ++r) {
        smore_ctx* c = g->ctx[r];
        auto& B = c->blk;
        (void)hipSetDevice(c->device);
        float* const* x = B.d_hub_ex;
        hipError_t e = hipSuccess;
        if (B.hub_pending) {
            e = hipStreamWaitEvent(c->stream, g->hdone[r], 0);
            if (e == hipSuccess)
                e = launch_delta_cycle_rows(hub_slots(c), x[0], x[1], x[2], B.d_hub_scale, (uint64_t)B.H, c->dpad,
                                            c->cus, c->stream);
        } else {
            e = launch_delta_begin(hub_slots(c), x[0], x[1], x[2], (uint64_t)B.H * c->dpad, c->cus, c->stream);
        }
        if (e == hipSuccess) e = hipEventRecord(g->hready[r], c->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(c->comm_stream, g->hready[r], 0);
        if (e != hipSuccess) return gfail(g, (int)r, fail(c, SMORE_EHIP, "hub exchange pass"));
        bufs.push_back(x[2]);
        st.push_back(c->comm_stream);
    }
    int rc;
    if ((rc = coll_allreduce(g, bufs, (size_t)g->ctx[0]->blk.H * g->ctx[0]->dpad, st, "hub ncclAllReduce"))) return rc;
    for (size_t r = 0; r < n; ++r) {
        (void)hipSetDevice(g->ctx[r]->device);
        if (hipEventRecord(g->hdone[r], g->ctx[r]->comm_stream) != hipSuccess)
            return gfail(g, (int)r, fail(g->ctx[r], SMORE_EHIP, "hub exchange: event"));
        g->ctx[r]->blk.hub_pending = true;
    }
    return SMORE_OK;
}

// the last exchange's end (every copy of the slots equal again), then the
// slots back into the hub rows, before block_finish gathers the blocks
int hub_ex_finish(smore_group* g) {
    if (!g->ctx[0]->blk.H) return SMORE_OK;
    for (size_t r = 0; r < g->ctx.size(); ++r) {
        smore_ctx* c = g->ctx[r];
        auto& B = c->blk;
        (void)hipSetDevice(c->device);
        if (B.hub_pending) {
            float* const* x = B.d_hub_ex;
            if (hipStreamWaitEvent(c->stream, g->hdone[r], 0) != hipSuccess ||
                launch_delta_end_rows(hub_slots(c), x[0], x[1], x[2], B.d_hub_scale, (uint64_t)B.H, c->dpad, c->cus,
                                      c->stream) != hipSuccess)
                return gfail(g, (int)r, fail(c, SMORE_EHIP, "hub exchange end"));
            B.hub_pending = false;
        }
        int rc;
        if ((rc = smore_block_hubs_store(c))) return gfail(g, (int)r, rc);
    }
    return SMORE_OK;
}

// SMORE_LOCAL_SERIAL=1 on a same-device group: replica r's next launch
// waits for the previous launch of replica r - 1 (of replica n - 1 for r = 0),
// so cells never share the GPU -- each runs with the whole device's
// concurrency, as on N GPUs (the quality studies' fidelity knob)
bool local_serial(const smore_group* g) {
    const char* e = getenv("SMORE_LOCAL_SERIAL");
    return g->local && e && atoi(e) != 0;
}

int serial_before(smore_group* g, size_t r) {
    if (!local_serial(g)) return SMORE_OK;
    const size_t n = g->ctx.size();
    if (g->lser.size() != n) {
        g->lser.assign(n, nullptr);
        for (size_t q = 0; q < n; ++q)
            if (hipEventCreateWithFlags(&g->lser[q], hipEventDisableTiming) != hipSuccess)
                return gfail(g, (int)q, fail(g->ctx[q], SMORE_EHIP, "serial events"));
        for (size_t q = 0; q < n; ++q) (void)hipEventRecord(g->lser[q], g->ctx[q]->stream);
    }
    const size_t p = (r + n - 1) % n;
    if (hipStreamWaitEvent(g->ctx[r]->stream, g->lser[p], 0) != hipSuccess)
        return gfail(g, (int)r, fail(g->ctx[r], SMORE_EHIP, "serial wait"));
    return SMORE_OK;
}

int serial_after(smore_group* g, size_t r) {
    if (!local_serial(g)) return SMORE_OK;
    if (hipEventRecord(g->lser[r], g->ctx[r]->stream) != hipSuccess)
        return gfail(g, (int)r, fail(g->ctx[r], SMORE_EHIP, "serial record"));
    return SMORE_OK;
}

// samples per row per replica per epoch of the LINE-2 block schedule (the C4
// bench's one epoch per 2^27-sample step: 13.4 per row)
constexpr double EDGE_BLOCK_PER_ROW = 13.42;
constexpr uint64_t WALK_BLOCK_ROUND = (uint64_t)1 << 18;   // walks per epoch (blocks.cpp's round cap)

// One epoch of cells: sub-round s trains cell (r, (2r + s) mod nb) on every
// replica r -- a cell in `launches` launches, the hub slots exchanged after
// each (blocks.cpp cell_launches) -- then after_sub(s) and the rotation.  S
// counts the call's sub-rounds; launch(r, block, q) queues launch q of
// replica r's cell on its stream and returns the replica's rc.
template <class Launch, class AfterSub>
int run_epoch_cells(smore_group* g, uint64_t& S, int launches, Launch&& launch, AfterSub&& after_sub) {
    const size_t n = g->ctx.size();
    const int nb = 2 * (int)n;
    int rc;
    for (int s = 0; s < nb; ++s, ++S) {
        for (int q = 0; q < launches; ++q) {
            for (size_t r = 0; r < n; ++r) {
                if (q == 0 && (rc = block_wait(g, r, S))) return rc;
                if ((rc = serial_before(g, r))) return rc;
                if ((rc = launch(r, (int)((2 * r + (size_t)s) % (size_t)nb), q))) return gfail(g, (int)r, rc);
                if ((rc = serial_after(g, r))) return rc;
            }
            if ((rc = hub_ex_post(g))) return rc;
        }
        after_sub(s);
        if ((rc = group_rotate(g, S))) return rc;
    }
    return SMORE_OK;
}

template <class Launch>
int run_epoch_cells(smore_group* g, uint64_t& S, int launches, Launch&& launch) {
    return run_epoch_cells(g, S, launches, launch, [](int) {});
}

}  // namespace

namespace smore_host {

int group_block_edges(smore_group* g, uint64_t begin, uint64_t count, uint64_t per, uint64_t total, int K,
                      double alpha0, uint64_t seed, int mode) {
    const size_t n = g->ctx.size();
    const int nb = 2 * (int)n;
    int rc;
    if (count == 0) return SMORE_OK;
    for (size_t r = 0; r < n; ++r)
        if ((rc = smore_block_setup(g->ctx[r], SMORE_LINE2, (int)n, (int)r, K, mode))) return gfail(g, (int)r, rc);
    if ((rc = ensure_block_events(g))) return rc;
    const int64_t V = g->ctx[0]->g->V;
    if (per == 0)
        per = (uint64_t)std::min(134217728.0, std::max(1024.0 * nb, std::round(EDGE_BLOCK_PER_ROW * (double)V)));
    const uint64_t round_units = per > count / n ? count : per * (uint64_t)n;
    const uint64_t rounds = (count + round_units - 1) / round_units;
    auto round_lo = [&](uint64_t k) { return (uint64_t)(((unsigned __int128)count * k) / rounds); };
    std::vector<std::vector<uint64_t>> cnt(n, std::vector<uint64_t>((size_t)nb));
    std::vector<uint64_t> cur(n), share(n);
    // a round's samples go to the replicas in proportion to their parts'
    // source mass, so the union of the parts draws SourceSample's law
    const std::vector<double>& pm = g->ctx[0]->blk.part_mass;
    const int split = cell_launches(g->ctx[0]->blk);
    if ((rc = hub_ex_start(g, (double)std::min<uint64_t>(per, count / n) / nb / split))) return rc;
    uint64_t S = 0;
    for (uint64_t k = 0; k < rounds; ++k) {
        const uint64_t lo = round_lo(k), m = round_lo(k + 1) - lo;
        largest_remainder(m, pm.data(), (int)n, share.data());
        uint64_t b = lo;
        for (size_t r = 0; r < n; ++r) {
            if ((rc = smore_block_counts(g->ctx[r], share[r], cnt[r].data()))) return gfail(g, (int)r, rc);
            cur[r] = b;
            b += share[r];
        }
        rc = run_epoch_cells(
            g, S, split,
            [&](size_t r, int bk, int q) {
                const uint64_t x0 = cnt[r][bk] * q / split, x = cnt[r][bk] * (q + 1) / split - x0;
                return x ? smore_block_train_edges_async(g->ctx[r], bk, begin + cur[r] + x0, x, total, K, alpha0, seed,
                                                         mode)
                         : SMORE_OK;
            },
            [&](int s) {
                for (size_t r = 0; r < n; ++r) cur[r] += cnt[r][(2 * r + (size_t)s) % (size_t)nb];
            });
        if (rc) return rc;
    }
    return block_finish(g, S);   // hub_ex_finish after the drain
}

int group_block_walks(smore_group* g, int rule, uint64_t walk_begin, uint64_t walk_end, int walk_times,
                      int walk_steps, int window, int window_min, int K, double alpha0, uint64_t seed,
                      const int64_t* order, int mode, uint64_t per) {
    const size_t n = g->ctx.size();
    const int nb = 2 * (int)n;
    int rc;
    const uint64_t total = (uint64_t)walk_times * (uint64_t)g->ctx[0]->g->V;
    if (walk_end > total) walk_end = total;
    if (walk_begin >= walk_end) return SMORE_OK;
    for (size_t r = 0; r < n; ++r)
        if ((rc = smore_block_setup(g->ctx[r], SMORE_CENSUS, (int)n, (int)r, K, mode))) return gfail(g, (int)r, rc);
    if ((rc = ensure_block_events(g))) return rc;
    if (per == 0 || per > WALK_BLOCK_ROUND) per = WALK_BLOCK_ROUND;
    {   // the hub slots' exchange: pair records per replica per sub-round
        const int L = walk_steps + 1;
        double ppw = 0.0;   // expected pairs per walk (SkipGrams' random shrink / Walklets' two ranges)
        for (int i = 0; i < L; ++i) {
            if (rule == 1) {
                ppw += (double)(std::min(L - 1, i + window) - std::min(L - 1, i + window_min - 1)) +
                       (double)(std::max(0, i - window_min + 1) - std::max(0, i - window));
            } else {
                for (int r = 1; r <= window; ++r)
                    ppw += (double)(std::min(L - 1, i + r) - std::max(0, i - r)) / window;
            }
        }
        const double walks = (double)std::min<uint64_t>(per, walk_end - walk_begin);
        const double launches = (double)cell_launches(g->ctx[0]->blk);
        if ((rc = hub_ex_start(g, std::max(1.0, walks * ppw / (double)(n * nb) / launches)))) return rc;
    }
    uint64_t S = 0;
    const char* ga = getenv("SMORE_WALK_GEN_ALL");
    const bool split_gen = !(ga && atoi(ga) != 0);
    for (uint64_t lo = walk_begin; lo < walk_end; lo += per) {
        const uint64_t hi = std::min(walk_end, lo + per), nw = hi - lo;
        // walk-partitioned generation: replica r walks its 1/N of the round,
        // every replica gets every walk (one broadcast of each slice from its
        // walker), then each buckets its own centres' pairs.  SMORE_WALK_GEN_ALL=1:
        // every replica walks every walk (round 5)
        for (size_t r = 0; r < n; ++r) {
            const uint64_t glo = split_gen ? lo + nw * r / n : lo, ghi = split_gen ? lo + nw * (r + 1) / n : hi;
            if ((rc = block_walks_gen(g->ctx[r], rule, lo, hi, glo, ghi, walk_times, walk_steps, window, window_min, K,
                                      alpha0, seed, order, 0, mode)))
                return gfail(g, (int)r, rc);
        }
        if (split_gen && n > 1) {
            const std::vector<hipStream_t> st = compute_streams(g);
            const size_t L = (size_t)walk_steps + 1;
            for (size_t q = 0; q < n; ++q) {
                const uint64_t o = nw * q / n, m = nw * (q + 1) / n - o;
                if (!m) continue;
                std::vector<float*> wb, lb;
                for (smore_ctx* c : g->ctx) {
                    wb.push_back(reinterpret_cast<float*>(c->d_walks + o * L));
                    lb.push_back(reinterpret_cast<float*>(c->d_lens + o));
                }
                if ((rc = coll_broadcast(g, wb, m * L, (int)q, st, "walks ncclBroadcast"))) return rc;
                if ((rc = coll_broadcast(g, lb, m, (int)q, st, "walk lengths ncclBroadcast"))) return rc;
            }
        }
        for (size_t r = 0; r < n; ++r)
            if ((rc = block_walks_emit(g->ctx[r]))) return gfail(g, (int)r, rc);
        const int L = cell_launches(g->ctx[0]->blk);
        rc = run_epoch_cells(g, S, L, [&](size_t r, int bk, int q) {
            return smore_block_train_walks_part_async(g->ctx[r], bk, q, L);
        });
        if (rc) return rc;
    }
    return block_finish(g, S);   // hub_ex_finish after the drain
}

}  // namespace smore_host

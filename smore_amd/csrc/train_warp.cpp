// train_warp.cpp -- the WARP driver of the C ABI (WARP::Train, src/model/
// WARP.cpp:55-108): per chunk of samples the draw kernel writes {v, i, j0}
// records (launch_draw with K = 1: slots 0-5 of the sample's unit, the prefix
// of the 4 + 2K layout), then warp_train_kernel runs the trial loop and draws
// the later negatives itself (warp_kernels.h).  The grid and the timing go
// through the record-launch path of train.cpp.
#include "train_host.h"

#include <algorithm>

using namespace smore_host;

// 1 / sum p_r^2 over a degree law: the number of equally likely rows with the
// same chance that two independent draws meet
static double effective_rows(const hvec<double>& deg) {
    double sum = 0.0, sq = 0.0;
    for (double d : deg) {
        sum += d;
        sq += d * d;
    }
    return sq > 0.0 ? sum * sum / sq : 1.0;
}

// Plain-store concurrency cap.  A group holds T[v] and T[i] in registers over
// its trial loop and stores whole rows, so of the groups in flight on one row
// all but one lose their update, and the rule grows the rows only through
// those updates.  R = the effective rows under the source law and the
// positive-item law; at most R / 32 groups run.  Measured on bip.txt (R = 32):
// two groups already cost 0.037 AUC, one group is the serial run (DESIGN.md
// 12a "Scatter quality").
static int64_t warp_store_groups(smore_ctx* c) {
    // tuning knob: SMORE_WARP_GROUPS sets the cap
    if (const char* e = getenv("SMORE_WARP_GROUPS"))
        if (atoll(e) > 0) return atoll(e);
    if (c->warp_rows <= 0.0) c->warp_rows = std::min(effective_rows(c->g->out_deg), effective_rows(c->g->in_deg));
    return std::max<int64_t>(1, (int64_t)(c->warp_rows / 32.0));
}

extern "C" {

int smore_train_warp_async(smore_ctx* c, uint64_t begin, uint64_t count, uint64_t total, double alpha0, uint64_t seed,
                           int mode) {
    if (!c) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (c->ntables < 1 || !c->d_table[0]) return fail(c, SMORE_ESTATE, "tables not allocated");
    if (int rc_ = refuse_cse(c)) return rc_;
    if (total == 0) return fail(c, SMORE_EINVAL, "total == 0");
    if (mode < 0 || mode > 3) return fail(c, SMORE_EINVAL, "bad mode");
    if (c->semantics == SMORE_SEM_GO) return fail(c, SMORE_EINVAL, "WARP has no Go semantics");
    if (c->census) return fail(c, SMORE_ESTATE, "row census: WARP's row rates depend on the tables (no census)");
    if (count == 0) return SMORE_OK;
    int rc;
    if ((rc = set_device(c))) return rc;
    if (!c->d_warp_stats) {
        HIPCHK(c, hipMalloc((void**)&c->d_warp_stats, 2 * sizeof(unsigned long long)));
        HIPCHK(c, hipMemset(c->d_warp_stats, 0, 2 * sizeof(unsigned long long)));
    }
    // the hybrid scatter is the atomic one here: no hot-row tags, no write-combining
    const int run_mode = mode == SMORE_HYBRID ? SMORE_ATOMIC : mode;
    constexpr int RW = rec_width(WARP_KMAX);
    uint64_t chunk_max = (uint64_t)1 << 27;
    if (const char* e = getenv("SMORE_DRAW_CHUNK")) chunk_max = std::max<uint64_t>(1024, strtoull(e, nullptr, 10));
    const uint64_t chunk = std::min<uint64_t>(count, chunk_max);
    const int nch = (int)((count + chunk - 1) / chunk);
    WarpArgs a{};
    a.sig = c->d_sig;
    a.T = c->d_table[0];
    a.work = c->d_work;
    a.stats = c->d_warp_stats;
    a.total = total;
    a.seed = seed;
    a.alpha0 = alpha0;
    a.dpad = c->dpad;
    a.mode = run_mode;
    const UpdateKernel kern = update_kernel(a);
    int grid = edge_grid(c, kern, run_mode, chunk);
    int groups = 256 / lanes_of(c->dpad);   // per block
    if (run_mode == SMORE_HOGWILD) {
        const int64_t cap = warp_store_groups(c);
        if (cap < groups) {
            grid = 1;
            groups = (int)cap;
        } else if (cap / groups < grid) {
            grid = (int)(cap / groups);
        }
    }
    if ((rc = ensure_cap(c, c->d_rec, c->rec_cap, chunk * RW))) return rc;
    if ((rc = grow_events(c, c->phase_ev, 2 * (size_t)nch + 1))) return rc;
    if ((rc = ensure_packed(c))) return rc;
    a.g = dev_graph(c);
    a.rec = c->d_rec;
    a.groups = groups;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    HIPCHK(c, hipEventRecord(c->phase_ev[0], c->stream));
    for (int k = 0; k < nch; ++k) {
        const uint64_t b = (uint64_t)k * chunk, n = std::min<uint64_t>(chunk, count - b);
        HIPCHK(c, launch_draw(a.g, seed, begin + b, n, 1, c->d_rec, c->d_skipped, c->stream));
        HIPCHK(c, hipEventRecord(c->phase_ev[2 * k + 1], c->stream));
        a.begin = begin + b;
        a.count = n;
        HIPCHK(c, hipMemsetAsync(c->d_work, 0, sizeof(unsigned long long), c->stream));
        HIPCHK(c, launch_update(kern, a, grid, c->stream));
        HIPCHK(c, hipEventRecord(c->phase_ev[2 * k + 2], c->stream));
    }
    return finish_timed(c, run_mode, nch);
}

int smore_train_warp(smore_ctx* c, uint64_t begin, uint64_t count, uint64_t total, double alpha0, uint64_t seed,
                     int mode) {
    return sync_after(c, smore_train_warp_async(c, begin, count, total, alpha0, seed, mode), true);
}

int smore_warp_stats(smore_ctx* c, uint64_t* trials, uint64_t* updated) {
    if (!c) return SMORE_EINVAL;
    unsigned long long h[2] = {0, 0};
    if (c->d_warp_stats) {
        int rc;
        if ((rc = set_device(c))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(h, c->d_warp_stats, sizeof(h), hipMemcpyDeviceToHost));
    }
    if (trials) *trials = h[0];
    if (updated) *updated = h[1];
    return SMORE_OK;
}

}  // extern "C"

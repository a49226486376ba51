// train_skewopt.cpp -- the Skew-OPT driver of the C ABI (SPR::Train, src/model/
// SkewOPT.cpp:55-110): per chunk of samples the draw kernel writes {v, i,
// j_0..j_15} records (launch_draw with K = 16: slots 0-35 of the sample's
// unit), then skewopt_train_kernel runs the sixteen negatives
// (skewopt_kernels.h).  The grid and the timing go through the record-launch
// path of train.cpp.
#include "train_host.h"

#include <algorithm>

using namespace smore_host;

extern "C" {

int smore_train_skewopt_async(smore_ctx* c, uint64_t begin, uint64_t count, uint64_t total, double alpha0, double xi,
                              double omega, int eta, uint64_t seed, int mode) {
    if (!c) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (c->ntables < 1 || !c->d_table[0]) return fail(c, SMORE_ESTATE, "tables not allocated");
    if (int rc_ = refuse_cse(c)) return rc_;
    if (total == 0) return fail(c, SMORE_EINVAL, "total == 0");
    if (mode < 0 || mode > 3) return fail(c, SMORE_EINVAL, "bad mode");
    if ((float)omega == 0.0f) return fail(c, SMORE_EINVAL, "omega == 0");
    if (eta < 1) return fail(c, SMORE_EINVAL, "eta < 1");
    if (mode == SMORE_HOGWILD)
        return fail(c, SMORE_EINVAL, "Skew-OPT has no plain-store scatter (whole-row stores lose colliding updates): "
                                     "use atomic, hybrid or serial");
    if (c->semantics == SMORE_SEM_GO) return fail(c, SMORE_EINVAL, "Skew-OPT has no Go semantics");
    if (c->census) return fail(c, SMORE_ESTATE, "row census: Skew-OPT's row rates depend on the tables (no census)");
    if (count == 0) return SMORE_OK;
    int rc;
    if ((rc = set_device(c))) return rc;
    if (!c->d_skewopt_stats) {
        HIPCHK(c, hipMalloc((void**)&c->d_skewopt_stats, 2 * sizeof(unsigned long long)));
        HIPCHK(c, hipMemset(c->d_skewopt_stats, 0, 2 * sizeof(unsigned long long)));
    }
    // the hybrid scatter is the atomic one here: no hot-row tags, no write-combining
    const int run_mode = mode == SMORE_HYBRID ? SMORE_ATOMIC : mode;
    constexpr int RW = rec_width(SKEWOPT_KMAX);
    uint64_t chunk_max = (uint64_t)1 << 25;   // 2^25 records of 128 B
    if (const char* e = getenv("SMORE_DRAW_CHUNK")) chunk_max = std::max<uint64_t>(1024, strtoull(e, nullptr, 10));
    const uint64_t chunk = std::min<uint64_t>(count, chunk_max);
    const int nch = (int)((count + chunk - 1) / chunk);
    SkewOptArgs a{};
    a.sig = c->d_sig;
    a.T = c->d_table[0];
    a.work = c->d_work;
    a.stats = c->d_skewopt_stats;
    a.total = total;
    a.alpha0 = alpha0;
    a.xi = (float)xi;
    a.omega = (float)omega;
    a.eta = eta;
    a.dpad = c->dpad;
    a.mode = run_mode;
    const UpdateKernel kern = update_kernel(a);
    const int grid = edge_grid(c, kern, run_mode, chunk);
    if ((rc = ensure_cap(c, c->d_rec, c->rec_cap, chunk * RW))) return rc;
    if ((rc = grow_events(c, c->phase_ev, 2 * (size_t)nch + 1))) return rc;
    if ((rc = ensure_packed(c))) return rc;
    const DevGraph g = dev_graph(c);
    a.rec = c->d_rec;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    HIPCHK(c, hipEventRecord(c->phase_ev[0], c->stream));
    for (int k = 0; k < nch; ++k) {
        const uint64_t b = (uint64_t)k * chunk, n = std::min<uint64_t>(chunk, count - b);
        HIPCHK(c, launch_draw(g, seed, begin + b, n, SKEW_NEG, c->d_rec, c->d_skipped, c->stream));
        HIPCHK(c, hipEventRecord(c->phase_ev[2 * k + 1], c->stream));
        a.begin = begin + b;
        a.count = n;
        HIPCHK(c, hipMemsetAsync(c->d_work, 0, sizeof(unsigned long long), c->stream));
        HIPCHK(c, launch_update(kern, a, grid, c->stream));
        HIPCHK(c, hipEventRecord(c->phase_ev[2 * k + 2], c->stream));
    }
    return finish_timed(c, run_mode, nch);
}

int smore_train_skewopt(smore_ctx* c, uint64_t begin, uint64_t count, uint64_t total, double alpha0, double xi,
                        double omega, int eta, uint64_t seed, int mode) {
    return sync_after(c, smore_train_skewopt_async(c, begin, count, total, alpha0, xi, omega, eta, seed, mode), true);
}

int smore_skewopt_stats(smore_ctx* c, uint64_t* passed, uint64_t* updated) {
    if (!c) return SMORE_EINVAL;
    unsigned long long h[2] = {0, 0};
    if (c->d_skewopt_stats) {
        int rc;
        if ((rc = set_device(c))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(h, c->d_skewopt_stats, sizeof(h), hipMemcpyDeviceToHost));
    }
    if (passed) *passed = h[0];
    if (updated) *updated = h[1];
    return SMORE_OK;
}

}  // extern "C"

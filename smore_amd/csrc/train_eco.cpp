// train_eco.cpp -- the sampled-softmax choice (ECO) rule in the C ABI: the driver
// ECO::Train (src/model/ECO.cpp:64-128) around proNet::UpdateDChoice
// (src/proNet.cpp:2221-2341), and ECO::Init's table (ECO.cpp:41-61).  Per chunk of
// samples eco_draw_kernel writes every row id of the sample and its clean flag
// (train_eco_draw.hip: the draws depend on the graph and the fields, never on
// the table), then eco_train_kernel runs the five lists (eco_kernels.h).  The
// grid and the timing go through the record-launch path of train.cpp.
#include "train_host.h"

using namespace smore_host;

// checks shared by the training and the dump entry; uploads the fields
static int eco_ready(smore_ctx* c, int K) {
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (K < 1 || K > ECO_MAX_K) return fail(c, SMORE_EINVAL, "negative_samples outside 1..20");
    if (c->semantics == SMORE_SEM_GO) return fail(c, SMORE_EINVAL, "ECO has no Go semantics");
    if (c->field.empty()) return fail(c, SMORE_ESTATE, "no fields (smore_load_field_meta / smore_set_fields)");
    if (c->field_src < 0) c->field_src = field0_has_source_mass(c) ? 1 : 0;
    if (!c->field_src) return fail(c, SMORE_ESTATE, "no field-0 vertex has source mass: no sample could start");
    int rc;
    if ((rc = set_device(c))) return rc;
    if (!c->d_field && (rc = upload(c, c->d_field, c->field.data(), c->field.size()))) return rc;
    return SMORE_OK;
}

extern "C" {

int smore_train_eco_async(smore_ctx* c, uint64_t begin, uint64_t count, uint64_t total, int negative_samples,
                          double alpha0, double reg, uint64_t seed, int mode) {
    if (!c) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (c->ntables < 1 || !c->d_table[0]) return fail(c, SMORE_ESTATE, "tables not allocated");
    if (int rc_ = refuse_cse(c)) return rc_;
    if (total == 0) return fail(c, SMORE_EINVAL, "total == 0");
    if (mode < 0 || mode > 3) return fail(c, SMORE_EINVAL, "bad mode");
    if (mode == SMORE_HOGWILD)
        return fail(c, SMORE_EINVAL, "ECO has no plain-store scatter (a row takes deltas, not values): "
                                     "use atomic, hybrid or serial");
    if (c->census) return fail(c, SMORE_ESTATE, "row census: ECO is not counted (no census)");
    int rc;
    if ((rc = eco_ready(c, negative_samples))) return rc;
    if (count == 0) return SMORE_OK;
    if (!c->d_eco_stats) {
        HIPCHK(c, hipMalloc((void**)&c->d_eco_stats, 2 * sizeof(unsigned long long)));
        HIPCHK(c, hipMemset(c->d_eco_stats, 0, 2 * sizeof(unsigned long long)));
    }
    // the hybrid scatter is the atomic one here: no hot-row tags, no write-combining
    const int run_mode = mode == SMORE_HYBRID ? SMORE_ATOMIC : mode;
    const uint64_t RW = (uint64_t)eco_width(negative_samples);
    uint64_t chunk_max = (uint64_t)1 << 22;   // 2^22 records of up to 448 B
    if (const char* e = getenv("SMORE_DRAW_CHUNK")) chunk_max = std::max<uint64_t>(1024, strtoull(e, nullptr, 10));
    const uint64_t chunk = std::min<uint64_t>(count, chunk_max);
    const int nch = (int)((count + chunk - 1) / chunk);
    EcoArgs a{};
    a.T = c->d_table[0];
    a.work = c->d_work;
    a.stats = c->d_eco_stats;
    a.total = total;
    a.alpha0 = alpha0;
    a.reg = (float)reg;
    a.dpad = c->dpad;
    a.mode = run_mode;
    a.K = negative_samples;
    const UpdateKernel kern = update_kernel(a);
    const int grid = edge_grid(c, kern, run_mode, chunk);
    if ((rc = ensure_cap(c, c->d_rec, c->rec_cap, chunk * RW))) return rc;
    if ((rc = ensure_cap(c, c->d_cbow_clean, c->cbow_clean_cap, chunk))) return rc;
    if ((rc = grow_events(c, c->phase_ev, 2 * (size_t)nch + 1))) return rc;
    const DevGraph g = dev_graph(c);
    a.rec = c->d_rec;
    a.clean = c->d_cbow_clean;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    HIPCHK(c, hipEventRecord(c->phase_ev[0], c->stream));
    for (int k = 0; k < nch; ++k) {
        const uint64_t b = (uint64_t)k * chunk, n = std::min<uint64_t>(chunk, count - b);
        HIPCHK(c, launch_eco_draw(g, c->d_field, seed, begin + b, n, negative_samples, c->d_rec, c->d_cbow_clean, nullptr,
                                  c->d_skipped, c->stream));
        HIPCHK(c, hipEventRecord(c->phase_ev[2 * k + 1], c->stream));
        a.begin = begin + b;
        a.count = n;
        HIPCHK(c, hipMemsetAsync(c->d_work, 0, sizeof(unsigned long long), c->stream));
        HIPCHK(c, launch_update(kern, a, grid, c->stream));
        HIPCHK(c, hipEventRecord(c->phase_ev[2 * k + 2], c->stream));
    }
    return finish_timed(c, run_mode, nch);
}

int smore_train_eco(smore_ctx* c, uint64_t begin, uint64_t count, uint64_t total, int negative_samples, double alpha0,
                    double reg, uint64_t seed, int mode) {
    return sync_after(c, smore_train_eco_async(c, begin, count, total, negative_samples, alpha0, reg, seed, mode), true);
}

int smore_eco_stats(smore_ctx* c, uint64_t* clean, uint64_t* ordered) {
    if (!c) return SMORE_EINVAL;
    unsigned long long h[2] = {0, 0};
    if (c->d_eco_stats) {
        int rc;
        if ((rc = set_device(c))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(h, c->d_eco_stats, sizeof(h), hipMemcpyDeviceToHost));
    }
    if (clean) *clean = h[0];
    if (ordered) *ordered = h[1];
    return SMORE_OK;
}

int smore_eco_records(smore_ctx* c, uint64_t begin, uint64_t count, int negative_samples, uint64_t seed, int32_t* out,
                      uint32_t* slots) {
    if (!c || !out) return SMORE_EINVAL;
    int rc;
    if ((rc = eco_ready(c, negative_samples))) return rc;
    if (count == 0) return SMORE_OK;
    const uint64_t RW = (uint64_t)eco_width(negative_samples);
    if ((rc = ensure_cap(c, c->d_rec, c->rec_cap, count * RW))) return rc;
    if ((rc = ensure_cap(c, c->d_cbow_clean, c->cbow_clean_cap, count))) return rc;
    if ((rc = ensure_cap(c, c->d_hoprec_slots, c->hoprec_slots_cap, count))) return rc;
    unsigned long long* d_skip = nullptr;   // a dump does not count into smore_skipped
    HIPCHK(c, hipMalloc((void**)&d_skip, sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d_skip, 0, sizeof(unsigned long long), c->stream);
    if (e == hipSuccess)
        e = launch_eco_draw(dev_graph(c), c->d_field, seed, begin, count, negative_samples, c->d_rec, c->d_cbow_clean,
                            c->d_hoprec_slots, d_skip, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, c->d_rec, count * RW * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && slots) e = hipMemcpy(slots, c->d_hoprec_slots, count * sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d_skip);
    if (e != hipSuccess) return fail(c, SMORE_EHIP, hipGetErrorString(e));
    return SMORE_OK;
}

int smore_init_table_glibc_unscaled(smore_ctx* c, int which, uint64_t skip, uint64_t stride) {
    int rc;
    if ((rc = check_table(c, which))) return rc;
    if (stride < 1) return fail(c, SMORE_EINVAL, "init_table_glibc_unscaled: stride >= 1");
    GlibcRand r;
    r.discard(skip);
    std::vector<float> h((size_t)c->g->V * c->dpad, 0.0f);
    for (int64_t v = 0; v < c->g->V; ++v)
        for (int d = 0; d < c->dim; ++d) {
            h[(size_t)v * c->dpad + d] = (float)(r.next() / (double)2147483647 - 0.5);
            r.discard(stride - 1);
        }
    if ((rc = set_device(c))) return rc;
    HIPCHK(c, hipMemcpy(c->d_table[which], h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return SMORE_OK;
}

}  // extern "C"

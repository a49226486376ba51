// train_cbowdev.cpp -- the bag-of-words event rule in the C ABI: the driver
// TEXTGCNdev::Train (src/model/TEXTGCNdev.cpp:71-126) around proNet::UpdateCBOWdev
// (src/proNet.cpp:2755-2865), and TEXTGCNdev::SaveWeights (TEXTGCNdev.cpp:6-39).  Per
// chunk of samples cbowdev_draw_kernel writes every row id of the sample and its
// clean flag (train_cbowdev_draw.hip: the draws depend on the fields, never on a
// table), then cbowdev_train_kernel runs the 12 num_events steps and the closing
// writes (cbowdev_kernels.h).  The grid and the timing go through the
// record-launch path of train.cpp.
#include "train_host.h"

using namespace smore_host;

// checks shared by the training and the dump entry; uploads the fields
static int cbowdev_ready(smore_ctx* c, int E, int N) {
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (E < 1 || E > CBOWDEV_MAX) return fail(c, SMORE_EINVAL, "num_events outside 1..10");
    if (N < 1 || N > CBOWDEV_MAX) return fail(c, SMORE_EINVAL, "num_words outside 1..10");
    if (c->semantics == SMORE_SEM_GO) return fail(c, SMORE_EINVAL, "CBOWdev has no Go semantics");
    if (c->field.empty()) return fail(c, SMORE_ESTATE, "no fields (smore_load_field_meta / smore_set_fields)");
    if (c->field_src < 0) c->field_src = field0_has_source_mass(c) ? 1 : 0;
    if (!c->field_src) return fail(c, SMORE_ESTATE, "no field-0 vertex has source mass: no sample could start");
    bool any1 = false;
    for (int32_t f : c->field) any1 = any1 || f == 1;
    if (!any1) return fail(c, SMORE_ESTATE, "no field-1 vertex: no negative could be drawn");
    int rc;
    if ((rc = set_device(c))) return rc;
    if (!c->d_field && (rc = upload(c, c->d_field, c->field.data(), c->field.size()))) return rc;
    return SMORE_OK;
}

extern "C" {

int smore_train_cbowdev_async(smore_ctx* c, uint64_t begin, uint64_t count, uint64_t total, int num_events,
                              int num_words, double alpha0, double reg, uint64_t seed, int mode) {
    if (!c) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (c->ntables < 1 || !c->d_table[0]) return fail(c, SMORE_ESTATE, "tables not allocated");
    if (c->ntables < 2 || !c->d_table[1]) return fail(c, SMORE_ESTATE, "CBOWdev needs W and C tables (no second table)");
    if (int rc_ = refuse_cse(c)) return rc_;
    if (total == 0) return fail(c, SMORE_EINVAL, "total == 0");
    if (mode < 0 || mode > 3) return fail(c, SMORE_EINVAL, "bad mode");
    if (mode == SMORE_HOGWILD)
        return fail(c, SMORE_EINVAL, "CBOWdev has no plain-store scatter (the bag rows take deltas, not values): "
                                     "use atomic, hybrid or serial");
    if (c->census) return fail(c, SMORE_ESTATE, "row census: CBOWdev is not counted (no census)");
    int rc;
    if ((rc = cbowdev_ready(c, num_events, num_words))) return rc;
    if (count == 0) return SMORE_OK;
    if (!c->d_cbowdev_stats) {
        HIPCHK(c, hipMalloc((void**)&c->d_cbowdev_stats, 2 * sizeof(unsigned long long)));
        HIPCHK(c, hipMemset(c->d_cbowdev_stats, 0, 2 * sizeof(unsigned long long)));
    }
    // the hybrid scatter is the atomic one here: no hot-row tags, no write-combining
    const int run_mode = mode == SMORE_HYBRID ? SMORE_ATOMIC : mode;
    const uint64_t RW = (uint64_t)cbowdev_width(num_events, num_words);
    uint64_t chunk_max = (uint64_t)1 << 22;   // 2^22 records of up to 816 B
    if (const char* e = getenv("SMORE_DRAW_CHUNK")) chunk_max = std::max<uint64_t>(1024, strtoull(e, nullptr, 10));
    const uint64_t chunk = std::min<uint64_t>(count, chunk_max);
    const int nch = (int)((count + chunk - 1) / chunk);
    CbowDevArgs a{};
    a.sig = c->d_sig;
    a.T = c->d_table[0];
    a.C = c->d_table[1];
    a.work = c->d_work;
    a.stats = c->d_cbowdev_stats;
    a.total = total;
    a.alpha0 = alpha0;
    a.reg = (float)reg;
    a.dpad = c->dpad;
    a.mode = run_mode;
    a.E = num_events;
    a.N = num_words;
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
        HIPCHK(c, launch_cbowdev_draw(g, c->d_field, seed, begin + b, n, num_events, num_words, c->d_rec, c->d_cbow_clean,
                                      nullptr, c->d_skipped, c->stream));
        HIPCHK(c, hipEventRecord(c->phase_ev[2 * k + 1], c->stream));
        a.begin = begin + b;
        a.count = n;
        HIPCHK(c, hipMemsetAsync(c->d_work, 0, sizeof(unsigned long long), c->stream));
        HIPCHK(c, launch_update(kern, a, grid, c->stream));
        HIPCHK(c, hipEventRecord(c->phase_ev[2 * k + 2], c->stream));
    }
    return finish_timed(c, run_mode, nch);
}

int smore_train_cbowdev(smore_ctx* c, uint64_t begin, uint64_t count, uint64_t total, int num_events, int num_words,
                        double alpha0, double reg, uint64_t seed, int mode) {
    return sync_after(c, smore_train_cbowdev_async(c, begin, count, total, num_events, num_words, alpha0, reg, seed, mode),
                      true);
}

int smore_cbowdev_stats(smore_ctx* c, uint64_t* clean, uint64_t* ordered) {
    if (!c) return SMORE_EINVAL;
    unsigned long long h[2] = {0, 0};
    if (c->d_cbowdev_stats) {
        int rc;
        if ((rc = set_device(c))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(h, c->d_cbowdev_stats, sizeof(h), hipMemcpyDeviceToHost));
    }
    if (clean) *clean = h[0];
    if (ordered) *ordered = h[1];
    return SMORE_OK;
}

int smore_cbowdev_records(smore_ctx* c, uint64_t begin, uint64_t count, int num_events, int num_words, uint64_t seed,
                          int32_t* out, uint32_t* slots) {
    if (!c || !out) return SMORE_EINVAL;
    int rc;
    if ((rc = cbowdev_ready(c, num_events, num_words))) return rc;
    if (count == 0) return SMORE_OK;
    const uint64_t RW = (uint64_t)cbowdev_width(num_events, num_words);
    if ((rc = ensure_cap(c, c->d_rec, c->rec_cap, count * RW))) return rc;
    if ((rc = ensure_cap(c, c->d_cbow_clean, c->cbow_clean_cap, count))) return rc;
    if ((rc = ensure_cap(c, c->d_hoprec_slots, c->hoprec_slots_cap, count))) return rc;
    unsigned long long* d_skip = nullptr;   // a dump does not count into smore_skipped
    HIPCHK(c, hipMalloc((void**)&d_skip, sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d_skip, 0, sizeof(unsigned long long), c->stream);
    if (e == hipSuccess)
        e = launch_cbowdev_draw(dev_graph(c), c->d_field, seed, begin, count, num_events, num_words, c->d_rec,
                                c->d_cbow_clean, c->d_hoprec_slots, d_skip, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, c->d_rec, count * RW * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && slots) e = hipMemcpy(slots, c->d_hoprec_slots, count * sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d_skip);
    if (e != hipSuccess) return fail(c, SMORE_EHIP, hipGetErrorString(e));
    return SMORE_OK;
}

int smore_save_weights_textgcndev(const smore_ctx* cc, const char* path, int fmt) {
    smore_ctx* c = const_cast<smore_ctx*>(cc);
    if (!c || !path) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (fmt != 0 && fmt != 1) return fail(c, SMORE_EINVAL, "save_weights_textgcndev: text formats only (0 %g, 1 %.6f)");
    if (c->field.empty()) return fail(c, SMORE_ESTATE, "no fields (smore_load_field_meta / smore_set_fields)");
    int rc;
    if ((rc = check_table(c, 0))) return rc;
    if ((rc = check_table(c, 1))) return rc;
    if ((rc = set_device(c))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const HostGraph& g = *c->g;
    std::vector<float> h[2];
    for (int t = 0; t < 2; ++t) {
        h[t].resize((size_t)g.V * c->dpad);
        HIPCHK(c, hipMemcpy(h[t].data(), c->d_table[t], h[t].size() * sizeof(float), hipMemcpyDeviceToHost));
    }
    FILE* f = fopen(path, "wb");
    if (!f) return fail(c, SMORE_EIO, std::string("cannot open ") + path);
    long long kept = 0;
    for (int64_t v = 0; v < g.V; ++v) kept += c->field[(size_t)v] != 1;
    fprintf(f, "%lld %d\n", kept, c->dim);
    std::string o;
    char num[64];
    bool ok = true;
    for (int64_t v = 0; ok && v < g.V; ++v) {
        const int32_t fv = c->field[(size_t)v];
        if (fv == 1) continue;
        o = g.names.empty() ? std::to_string((long long)v) : g.names[(size_t)v];
        if (fv == 0 || fv == 2) {
            // field 0: the w_vertex row, field 2: the w_context row
            const float* r = h[fv == 0 ? 0 : 1].data() + (size_t)v * c->dpad;
            for (int d = 0; d < c->dim; ++d)
                o.append(num, (size_t)snprintf(num, sizeof num, fmt == 1 ? " %.6f" : " %g", (double)r[d]));
        }
        o.push_back('\n');
        ok = fwrite(o.data(), 1, o.size(), f) == o.size();
    }
    ok = (fclose(f) == 0) && ok;
    return ok ? SMORE_OK : fail(c, SMORE_EIO, std::string("write failed: ") + path);
}

}  // extern "C"

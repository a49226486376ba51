// train_cse.cpp -- CSE (nemf, nerank) in the C ABI: the driver (NEMF::Train,
// src/model/NEMF.cpp:87-149, NERANK::Train, src/model/NERANK.cpp:87-148), Init's
// interleaved table fill (NEMF.cpp:62-70) and the per-field SaveWeights
// (NEMF.cpp:21-47).  A CSE context has four tables WU, WI, CU, CI
// (smore_alloc_tables with ntables 4).  Per chunk of samples cse_draw_kernel
// writes every row id of the sample (train_cse_draw.hip: the draws depend on
// the fields, never on the tables), then cse_train_kernel runs the two passes
// and the direct term (cse_kernels.h).  The grid and the timing go through the
// record-launch path of train.cpp.
#include "train_host.h"

using namespace smore_host;

// checks shared by the training and the dump entry; uploads the fields
static int cse_ready(smore_ctx* c, int rank, int walk_steps) {
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (rank != 0 && rank != 1) return fail(c, SMORE_EINVAL, "rank: 0 nemf, 1 nerank");
    if (walk_steps < 1 || walk_steps > CSE_MAX_STEPS) return fail(c, SMORE_EINVAL, "walk_steps outside 1..10");
    if (c->semantics == SMORE_SEM_GO) return fail(c, SMORE_EINVAL, "CSE has no Go semantics");
    if (c->field.empty()) return fail(c, SMORE_ESTATE, "no fields (smore_load_field_meta / smore_set_fields)");
    if (c->field_src < 0) c->field_src = field0_has_source_mass(c) ? 1 : 0;
    if (!c->field_src) return fail(c, SMORE_ESTATE, "no field-0 vertex has source mass: no sample could start");
    int rc;
    if ((rc = set_device(c))) return rc;
    if (!c->d_field && (rc = upload(c, c->d_field, c->field.data(), c->field.size()))) return rc;
    return SMORE_OK;
}

extern "C" {

int smore_init_tables_glibc_pair(smore_ctx* c, int a, int b, uint64_t skip) {
    int rc;
    if ((rc = check_table(c, a)) || (rc = check_table(c, b))) return rc;
    if (a == b) return fail(c, SMORE_EINVAL, "init_tables_glibc_pair: two different tables");
    GlibcRand r;
    r.discard(skip);
    const size_t n = (size_t)c->g->V * c->dpad;
    std::vector<float> ha(n, 0.0f), hb(n, 0.0f);
    // one rand() stream, per element table a then table b (NEMF::Init)
    for (int64_t v = 0; v < c->g->V; ++v)
        for (int d = 0; d < c->dim; ++d) {
            ha[(size_t)v * c->dpad + d] = (float)((r.next() / (double)2147483647 - 0.5) / c->dim);
            hb[(size_t)v * c->dpad + d] = (float)((r.next() / (double)2147483647 - 0.5) / c->dim);
        }
    if ((rc = set_device(c))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(c->d_table[a], ha.data(), n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_table[b], hb.data(), n * sizeof(float), hipMemcpyHostToDevice));
    return SMORE_OK;
}

int smore_save_weights_fields(const smore_ctx* cc, const int* table_of_field, int nfields, const char* path, int fmt) {
    smore_ctx* c = const_cast<smore_ctx*>(cc);
    if (!c || !table_of_field || !path) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (fmt != 0 && fmt != 1) return fail(c, SMORE_EINVAL, "save_weights_fields: text formats only (0 %g, 1 %.6f)");
    if (c->field.empty()) return fail(c, SMORE_ESTATE, "no fields (smore_load_field_meta / smore_set_fields)");
    if (nfields < c->nfields) return fail(c, SMORE_EINVAL, "save_weights_fields: a table (or -1) for every field");
    int rc;
    bool used[4] = {false, false, false, false};
    for (int f = 0; f < c->nfields; ++f) {
        if (table_of_field[f] < -1 || table_of_field[f] > 3) return fail(c, SMORE_EINVAL, "save_weights_fields: bad table");
        if (table_of_field[f] >= 0) {
            if ((rc = check_table(c, table_of_field[f]))) return rc;
            used[table_of_field[f]] = true;
        }
    }
    if ((rc = set_device(c))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const HostGraph& g = *c->g;
    std::vector<float> h[4];
    for (int t = 0; t < 4; ++t)
        if (used[t]) {
            h[t].resize((size_t)g.V * c->dpad);
            HIPCHK(c, hipMemcpy(h[t].data(), c->d_table[t], h[t].size() * sizeof(float), hipMemcpyDeviceToHost));
        }
    FILE* f = fopen(path, "wb");
    if (!f) return fail(c, SMORE_EIO, std::string("cannot open ") + path);
    fprintf(f, "%lld %d\n", (long long)g.V, c->dim);
    std::string o;
    char num[64];
    bool ok = true;
    for (int64_t v = 0; ok && v < g.V; ++v) {
        o = g.names.empty() ? std::to_string((long long)v) : g.names[(size_t)v];
        const int t = table_of_field[c->field[(size_t)v]];
        if (t >= 0) {
            const float* r = h[t].data() + (size_t)v * c->dpad;
            for (int d = 0; d < c->dim; ++d) o.append(num, (size_t)snprintf(num, sizeof num, fmt == 1 ? " %.6f" : " %g", (double)r[d]));
        }
        o.push_back('\n');
        ok = fwrite(o.data(), 1, o.size(), f) == o.size();
    }
    ok = (fclose(f) == 0) && ok;
    return ok ? SMORE_OK : fail(c, SMORE_EIO, std::string("write failed: ") + path);
}

int smore_train_cse_async(smore_ctx* c, int rank, uint64_t begin, uint64_t count, uint64_t total, int walk_steps,
                          double alpha0, uint64_t seed, int mode) {
    if (!c) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (c->ntables != 4 || !c->d_table[3])
        return fail(c, SMORE_ESTATE, "CSE needs four tables WU, WI, CU, CI (smore_alloc_tables with ntables 4)");
    if (total == 0) return fail(c, SMORE_EINVAL, "total == 0");
    if (mode < 0 || mode > 3) return fail(c, SMORE_EINVAL, "bad mode");
    if (mode == SMORE_HOGWILD)
        return fail(c, SMORE_EINVAL, "CSE has no plain-store scatter (whole-row stores lose colliding updates): "
                                     "use atomic, hybrid or serial");
    if (c->census) return fail(c, SMORE_ESTATE, "row census: CSE's row rates depend on the tables (no census)");
    int rc;
    if ((rc = cse_ready(c, rank, walk_steps))) return rc;
    if (count == 0) return SMORE_OK;
    if (!c->d_cse_stats) {
        HIPCHK(c, hipMalloc((void**)&c->d_cse_stats, 2 * sizeof(unsigned long long)));
        HIPCHK(c, hipMemset(c->d_cse_stats, 0, 2 * sizeof(unsigned long long)));
    }
    // the hybrid scatter is the atomic one here: no hot-row tags, no write-combining
    const int run_mode = mode == SMORE_HYBRID ? SMORE_ATOMIC : mode;
    const uint64_t RW = (uint64_t)cse_width(walk_steps, rank);
    uint64_t chunk_max = (uint64_t)1 << 22;   // 2^22 records of up to 544 B
    if (const char* e = getenv("SMORE_DRAW_CHUNK")) chunk_max = std::max<uint64_t>(1024, strtoull(e, nullptr, 10));
    const uint64_t chunk = std::min<uint64_t>(count, chunk_max);
    const int nch = (int)((count + chunk - 1) / chunk);
    CseArgs a{};
    a.sig = c->d_sig;
    for (int t = 0; t < 4; ++t) a.T[t] = c->d_table[t];
    a.work = c->d_work;
    a.stats = c->d_cse_stats;
    a.total = total;
    a.alpha0 = alpha0;
    a.dpad = c->dpad;
    a.mode = run_mode;
    a.steps = walk_steps;
    a.rank = rank;
    const UpdateKernel kern = update_kernel(a);
    const int grid = edge_grid(c, kern, run_mode, chunk);
    if ((rc = ensure_cap(c, c->d_rec, c->rec_cap, chunk * RW))) return rc;
    if ((rc = grow_events(c, c->phase_ev, 2 * (size_t)nch + 1))) return rc;
    const DevGraph g = dev_graph(c);
    a.rec = c->d_rec;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    HIPCHK(c, hipEventRecord(c->phase_ev[0], c->stream));
    for (int k = 0; k < nch; ++k) {
        const uint64_t b = (uint64_t)k * chunk, n = std::min<uint64_t>(chunk, count - b);
        HIPCHK(c, launch_cse_draw(g, c->d_field, seed, begin + b, n, walk_steps, rank, c->d_rec, nullptr, c->d_skipped,
                                  c->stream));
        HIPCHK(c, hipEventRecord(c->phase_ev[2 * k + 1], c->stream));
        a.begin = begin + b;
        a.count = n;
        HIPCHK(c, hipMemsetAsync(c->d_work, 0, sizeof(unsigned long long), c->stream));
        HIPCHK(c, launch_update(kern, a, grid, c->stream));
        HIPCHK(c, hipEventRecord(c->phase_ev[2 * k + 2], c->stream));
    }
    return finish_timed(c, run_mode, nch);
}

int smore_train_cse(smore_ctx* c, int rank, uint64_t begin, uint64_t count, uint64_t total, int walk_steps,
                    double alpha0, uint64_t seed, int mode) {
    return sync_after(c, smore_train_cse_async(c, rank, begin, count, total, walk_steps, alpha0, seed, mode), true);
}

int smore_cse_stats(smore_ctx* c, uint64_t* tested, uint64_t* updated) {
    if (!c) return SMORE_EINVAL;
    unsigned long long h[2] = {0, 0};
    if (c->d_cse_stats) {
        int rc;
        if ((rc = set_device(c))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(h, c->d_cse_stats, sizeof(h), hipMemcpyDeviceToHost));
    }
    if (tested) *tested = h[0];
    if (updated) *updated = h[1];
    return SMORE_OK;
}

int smore_cse_records(smore_ctx* c, int rank, uint64_t begin, uint64_t count, int walk_steps, uint64_t seed,
                      int32_t* out, uint32_t* slots) {
    if (!c || !out) return SMORE_EINVAL;
    int rc;
    if ((rc = cse_ready(c, rank, walk_steps))) return rc;
    if (count == 0) return SMORE_OK;
    const uint64_t RW = (uint64_t)cse_width(walk_steps, rank);
    if ((rc = ensure_cap(c, c->d_rec, c->rec_cap, count * RW))) return rc;
    if ((rc = ensure_cap(c, c->d_hoprec_slots, c->hoprec_slots_cap, count))) return rc;
    unsigned long long* d_skip = nullptr;   // a dump does not count into smore_skipped
    HIPCHK(c, hipMalloc((void**)&d_skip, sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d_skip, 0, sizeof(unsigned long long), c->stream);
    if (e == hipSuccess)
        e = launch_cse_draw(dev_graph(c), c->d_field, seed, begin, count, walk_steps, rank, c->d_rec, c->d_hoprec_slots,
                            d_skip, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, c->d_rec, count * RW * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && slots) e = hipMemcpy(slots, c->d_hoprec_slots, count * sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d_skip);
    if (e != hipSuccess) return fail(c, SMORE_EHIP, hipGetErrorString(e));
    return SMORE_OK;
}

}  // extern "C"

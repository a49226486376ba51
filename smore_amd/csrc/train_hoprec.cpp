// train_hoprec.cpp -- HOP-REC in the C ABI: the vertex fields
// (proNet::LoadFieldMeta, src/proNet.cpp:330-408; only fields[0], no vids
// lists) and the driver (HBPR::Train, src/model/HBPR.cpp:63-131).  Per chunk
// of samples hoprec_draw_kernel writes every sample's 1 + 6 walk_steps row ids
// (train_hoprec_draw.hip: the draws depend on the fields, never on the
// tables), then hoprec_train_kernel runs the steps (hoprec_kernels.h).  The
// grid and the timing go through the record-launch path of train.cpp.
#include <unordered_map>

#include "train_host.h"

using namespace smore_host;

// a field-0 vertex can come out of SourceSample: some alias entry returns it
bool smore_host::field0_has_source_mass(const smore_ctx* c) {
    const HostGraph& g = *c->g;
    for (int64_t i = 0; i < g.V; ++i) {
        const AliasEntry& e = g.vtab[i];
        if (e.thresh > 0 && c->field[i] == 0) return true;
        if (e.thresh != 0xFFFFFFFFu && c->field[e.alias & ID_MASK] == 0) return true;   // the alias word carries tags
    }
    return false;
}

static int set_fields(smore_ctx* c, std::vector<int32_t>&& f, int nfields) {
    c->field = std::move(f);
    c->nfields = nfields;
    c->field_src = -1;
    if (c->device >= 0) {
        int rc;
        if ((rc = set_device(c))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));   // a training call may still read the old copy
    }
    dfree(c->d_field);
    return SMORE_OK;
}

// checks shared by the training and the dump entry; uploads the fields
static int hoprec_ready(smore_ctx* c, int walk_steps) {
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (walk_steps < 1 || walk_steps > HOPREC_MAX_STEPS) return fail(c, SMORE_EINVAL, "walk_steps outside 1..10");
    if (c->semantics == SMORE_SEM_GO) return fail(c, SMORE_EINVAL, "HOP-REC has no Go semantics");
    if (c->field.empty()) return fail(c, SMORE_ESTATE, "no fields (smore_load_field_meta / smore_set_fields)");
    if (c->field_src < 0) c->field_src = field0_has_source_mass(c) ? 1 : 0;
    if (!c->field_src) return fail(c, SMORE_ESTATE, "no field-0 vertex has source mass: no sample could start");
    int rc;
    if ((rc = set_device(c))) return rc;
    if (!c->d_field && (rc = upload(c, c->d_field, c->field.data(), c->field.size()))) return rc;
    return SMORE_OK;
}

extern "C" {

int smore_set_fields(smore_ctx* c, const int32_t* field, int nfields) {
    if (!c || !field || nfields < 1) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    const int64_t V = c->g->V;
    for (int64_t v = 0; v < V; ++v)
        if (field[v] < 0 || field[v] >= nfields) return fail(c, SMORE_EINVAL, "field out of range");
    return set_fields(c, std::vector<int32_t>(field, field + V), nfields);
}

int smore_get_fields(const smore_ctx* c, int32_t* field, int* nfields) {
    if (!c) return SMORE_EINVAL;
    if (nfields) *nfields = c->nfields;
    if (field && !c->field.empty()) std::copy(c->field.begin(), c->field.end(), field);
    return SMORE_OK;
}

int smore_load_field_meta(smore_ctx* c, const char* path) {
    if (!c || !path) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    const HostGraph& g = *c->g;
    if (g.names.empty()) return fail(c, SMORE_ESTATE, "field meta needs vertex names (load an edge list)");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(c, SMORE_EIO, std::string("cannot open ") + path);
    std::unordered_map<std::string, int32_t> ids, meta;
    ids.reserve(g.names.size());
    for (size_t i = 0; i < g.names.size(); ++i) ids.emplace(g.names[i], (int32_t)i);
    std::vector<int32_t> field((size_t)g.V, 0);   // a vertex the file does not name keeps field 0
    int64_t lines = 0, unknown = 0;
    char name[160], m[160];
    // "%s %s" pairs as the reference reads them; a field's id is its order of
    // first appearance, given before the name is looked up (:368-377)
    while (fscanf(f, "%159s %159s", name, m) == 2) {
        const int32_t id = meta.emplace(m, (int32_t)meta.size()).first->second;
        const auto it = ids.find(name);
        lines++;
        if (it == ids.end()) {   // "vertex ... is not in given network": counted, smore_field_meta_info
            unknown++;
            continue;
        }
        field[(size_t)it->second] = id;
    }
    fclose(f);
    if (meta.empty()) return fail(c, SMORE_EIO, std::string("no field lines in ") + path);
    c->field_lines = lines;
    c->field_unknown = unknown;
    return set_fields(c, std::move(field), (int)meta.size());
}

int smore_field_meta_info(const smore_ctx* c, int64_t* lines, int64_t* unknown) {
    if (!c) return SMORE_EINVAL;
    if (lines) *lines = c->field_lines;
    if (unknown) *unknown = c->field_unknown;
    return SMORE_OK;
}

int smore_train_hoprec_async(smore_ctx* c, uint64_t begin, uint64_t count, uint64_t total, int walk_steps,
                             double alpha0, uint64_t seed, int mode) {
    if (!c) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (c->ntables < 1 || !c->d_table[0]) return fail(c, SMORE_ESTATE, "tables not allocated");
    if (int rc_ = refuse_cse(c)) return rc_;
    if (total == 0) return fail(c, SMORE_EINVAL, "total == 0");
    if (mode < 0 || mode > 3) return fail(c, SMORE_EINVAL, "bad mode");
    if (mode == SMORE_HOGWILD)
        return fail(c, SMORE_EINVAL, "HOP-REC has no plain-store scatter (whole-row stores lose colliding updates): "
                                     "use atomic, hybrid or serial");
    if (c->census) return fail(c, SMORE_ESTATE, "row census: HOP-REC's row rates depend on the tables (no census)");
    int rc;
    if ((rc = hoprec_ready(c, walk_steps))) return rc;
    if (count == 0) return SMORE_OK;
    if (!c->d_hoprec_stats) {
        HIPCHK(c, hipMalloc((void**)&c->d_hoprec_stats, 2 * sizeof(unsigned long long)));
        HIPCHK(c, hipMemset(c->d_hoprec_stats, 0, 2 * sizeof(unsigned long long)));
    }
    // the hybrid scatter is the atomic one here: no hot-row tags, no write-combining
    const int run_mode = mode == SMORE_HYBRID ? SMORE_ATOMIC : mode;
    const uint64_t RW = (uint64_t)hoprec_width(walk_steps);
    uint64_t chunk_max = (uint64_t)1 << 24;   // 2^24 records of up to 256 B
    if (const char* e = getenv("SMORE_DRAW_CHUNK")) chunk_max = std::max<uint64_t>(1024, strtoull(e, nullptr, 10));
    const uint64_t chunk = std::min<uint64_t>(count, chunk_max);
    const int nch = (int)((count + chunk - 1) / chunk);
    HopRecArgs a{};
    a.sig = c->d_sig;
    a.T = c->d_table[0];
    a.work = c->d_work;
    a.stats = c->d_hoprec_stats;
    a.total = total;
    a.alpha0 = alpha0;
    a.dpad = c->dpad;
    a.mode = run_mode;
    a.steps = walk_steps;
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
        HIPCHK(c, launch_hoprec_draw(g, c->d_field, seed, begin + b, n, walk_steps, c->d_rec, nullptr, c->d_skipped,
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

int smore_train_hoprec(smore_ctx* c, uint64_t begin, uint64_t count, uint64_t total, int walk_steps, double alpha0,
                       uint64_t seed, int mode) {
    return sync_after(c, smore_train_hoprec_async(c, begin, count, total, walk_steps, alpha0, seed, mode), true);
}

int smore_hoprec_stats(smore_ctx* c, uint64_t* tested, uint64_t* passed) {
    if (!c) return SMORE_EINVAL;
    unsigned long long h[2] = {0, 0};
    if (c->d_hoprec_stats) {
        int rc;
        if ((rc = set_device(c))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(h, c->d_hoprec_stats, sizeof(h), hipMemcpyDeviceToHost));
    }
    if (tested) *tested = h[0];
    if (passed) *passed = h[1];
    return SMORE_OK;
}

int smore_hoprec_records(smore_ctx* c, uint64_t begin, uint64_t count, int walk_steps, uint64_t seed, int32_t* out,
                         uint32_t* slots) {
    if (!c || !out) return SMORE_EINVAL;
    int rc;
    if ((rc = hoprec_ready(c, walk_steps))) return rc;
    if (count == 0) return SMORE_OK;
    const uint64_t RW = (uint64_t)hoprec_width(walk_steps);
    if ((rc = ensure_cap(c, c->d_rec, c->rec_cap, count * RW))) return rc;
    if ((rc = ensure_cap(c, c->d_hoprec_slots, c->hoprec_slots_cap, count))) return rc;
    unsigned long long* d_skip = nullptr;   // a dump does not count into smore_skipped
    HIPCHK(c, hipMalloc((void**)&d_skip, sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d_skip, 0, sizeof(unsigned long long), c->stream);
    if (e == hipSuccess)
        e = launch_hoprec_draw(dev_graph(c), c->d_field, seed, begin, count, walk_steps, c->d_rec, c->d_hoprec_slots,
                               d_skip, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, c->d_rec, count * RW * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && slots) e = hipMemcpy(slots, c->d_hoprec_slots, count * sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d_skip);
    if (e != hipSuccess) return fail(c, SMORE_EHIP, hipGetErrorString(e));
    // the ids as vertex numbers (the hot tag is the update kernel's business)
    for (uint64_t k = 0; k < count * RW; ++k)
        if (out[k] >= 0) out[k] &= ID_MASK;
    return SMORE_OK;
}

}  // extern "C"

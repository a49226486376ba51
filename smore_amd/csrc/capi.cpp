// capi.cpp -- the C ABI (include/smore_hip.h) over the gfx950 kernels: the
// context, its graph and tables.  The source partition and the hot-row policy
// are in hot_maps.cpp, the training drivers in train.cpp, the row transfers
// and the multi-caller combiner in pairs_rows.cpp, the block schedule in
// blocks.cpp and block_plan.cpp, the replica exchange in exchange.cpp, the
// one-process group in group.cpp and group_blocks.cpp.
//
// A context owns one GPU's copy of the graph (CSR, encoded alias tables, the
// fastSigmoid table) and the embedding tables.  Everything on the device is
// uploaded once; training calls only launch kernels on the context stream.
#include "hot_exchange.h"
#include "train_host.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

using namespace smore_host;

extern "C" {

const char* smore_version(void) { return "smore_hip 0.1 (gfx950)"; }

int smore_create(int device, smore_ctx** out) {
    if (!out) return SMORE_EINVAL;
    *out = nullptr;
    smore_ctx* c = new smore_ctx();
    c->device = device;
    if (device < 0) {  // host-only context: graph/alias building, no device state
        *out = c;
        return SMORE_OK;
    }
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->draw_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_skipped, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(c->d_skipped, 0, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_work, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) {
        delete c;
        return SMORE_EHIP;
    }
    c->stream = c->own_stream;
    *out = c;
    return SMORE_OK;
}

void smore_destroy(smore_ctx* c) {
    if (!c) return;
    smore_exchange_release(c);
    if (c->device >= 0) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
    }
    dfree(c->d_offsets); dfree(c->d_targets); dfree(c->d_vtab); dfree(c->d_ntab); dfree(c->d_ctab);
    dfree(c->d_sig); dfree(c->d_skipped); dfree(c->d_work); dfree(c->d_warp_stats); dfree(c->d_field); dfree(c->d_hoprec_slots); dfree(c->d_hoprec_stats); dfree(c->d_skewopt_stats); dfree(c->d_cse_stats); dfree(c->d_cbow_stats); dfree(c->d_cbow_clean); dfree(c->d_eco_stats); dfree(c->d_cbowdev_stats);
    for (float*& t : c->d_table) dfree(t);

    dfree(c->d_order); dfree(c->d_walks); dfree(c->d_lens); dfree(c->d_tcum); dfree(c->d_wts); dfree(c->d_nbr_sorted); dfree(c->d_ntype); dfree(c->d_ttargets); dfree(c->d_toff); dfree(c->d_paths); dfree(c->d_path_off); dfree(c->d_t_off); dfree(c->d_t_tgt); dfree(c->d_t_ts); dfree(c->d_t_min); dfree(c->d_t_max); dfree(c->d_sh_hash); dfree(c->d_sh_ids);
    dfree(c->d_rec); dfree(c->d_vt32); dfree(c->d_ct16); dfree(c->d_split);
    dfree(c->d_pcount); dfree(c->d_poff); dfree(c->d_pairs); dfree(c->d_census[0]); dfree(c->d_census[1]);
    dfree(c->d_io_ids[0]); dfree(c->d_io_rows[0]); dfree(c->d_io_ids[1]); dfree(c->d_io_rows[1]);
    blocks_release(c);
    if (c->d_scan_tmp) (void)hipFree(c->d_scan_tmp);
    for (hipEvent_t e : c->phase_ev) (void)hipEventDestroy(e);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->draw_stream) (void)hipStreamDestroy(c->draw_stream);
    for (hipEvent_t e : c->sync_ev) (void)hipEventDestroy(e);
    delete c;
}

const char* smore_last_error(const smore_ctx* c) { return c ? c->err.c_str() : "null context"; }

int smore_set_stream(smore_ctx* c, void* s) {
    if (!c) return SMORE_EINVAL;
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return SMORE_OK;
}

int smore_synchronize(smore_ctx* c) {
    if (!c) return SMORE_EINVAL;
    if (c->device < 0) return SMORE_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = comm_sync(c))) return rc;   // own communicator: the RCCL failure watch first
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SMORE_OK;
}

// ---------------------------------------------------------------- graph
int smore_set_graph_edges(smore_ctx* c, int64_t V, int64_t E, const int32_t* src, const int32_t* dst,
                          const double* w, int vm, int nm) {
    if (!c) return SMORE_EINVAL;
    if ((E > 0 && (!src || !dst || !w)) || vm < 0 || vm > 2 || nm < 0 || nm > 2)
        return fail(c, SMORE_EINVAL, "bad arguments");
    c->g = std::make_shared<HostGraph>();
    c->hot_key.clear();
    c->semantics = SMORE_SEM_CPP;
    if (!build_graph(V, E, src, dst, w, vm, nm, *c->g, c->err)) return SMORE_EINVAL;
    return upload_graph(c);
}

int smore_load_edgelist(smore_ctx* c, const char* path, int undirected, int vm, int nm) {
    if (!c || !path) return SMORE_EINVAL;
    if (vm < 0 || vm > 2 || nm < 0 || nm > 2) return fail(c, SMORE_EINVAL, "bad arguments");
    std::vector<std::string> names;
    std::vector<int32_t> src, dst;
    std::vector<double> w;
    const char* cache = !c->cache_dir.empty() ? c->cache_dir.c_str() : getenv("SMORE_CACHE_DIR");
    const auto t0 = std::chrono::steady_clock::now();
    // with a cache directory: the built graph of this input and these methods,
    // if an earlier load stored it (no parse, no CSR / alias build)
    std::string gfile;
    uint64_t key = 0;
    if (cache && *cache && edgelist_key(path, undirected != 0, &key, c->err)) {
        char name[96];
        snprintf(name, sizeof name, "/%016llx-v%dn%d.smoregc", (unsigned long long)key, vm, nm);
        gfile = std::string(cache) + name;
        auto g = std::make_shared<HostGraph>();
        if (load_graph_cache(gfile, key, vm, nm, *g)) {
            c->g = g;
            c->hot_key.clear();
            c->semantics = SMORE_SEM_CPP;
            c->load_stats = LoadStats();
            c->load_stats.cache_hit = 2;
            c->load_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            return upload_graph(c);
        }
    }
    if (!read_edgelist(path, undirected != 0, names, src, dst, w, c->err, cache, &c->load_stats)) return SMORE_EIO;
    c->load_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (names.empty()) return fail(c, SMORE_EIO, std::string("no edges in ") + path);
    int rc = smore_set_graph_edges(c, (int64_t)names.size(), (int64_t)src.size(), src.data(), dst.data(),
                                   w.data(), vm, nm);
    if (rc == SMORE_OK) c->g->names = std::move(names);
    if (rc == SMORE_OK && !gfile.empty()) (void)save_graph_cache(gfile, key, *c->g);
    return rc;
}

// the built graph (CSR, degrees, alias tables) to / from a binary file: one
// process of a multi-GPU job builds it, the others read it (bench.py at N > 1;
// the same format as the edge-list loader's graph cache, loader.cpp)
static constexpr uint64_t GRAPH_FILE_KEY = 0x534d4f5245475246ull;   // "SMOREGRF"

int smore_save_graph(const smore_ctx* c, const char* path) {
    if (!c || !path) return SMORE_EINVAL;
    if (!c->has_graph) return SMORE_ESTATE;
    return save_graph_cache(path, GRAPH_FILE_KEY, *c->g) ? SMORE_OK : SMORE_EIO;
}

int smore_load_graph(smore_ctx* c, const char* path, int vm, int nm) {
    if (!c || !path || vm < 0 || vm > 2 || nm < 0 || nm > 2) return SMORE_EINVAL;
    auto g = std::make_shared<HostGraph>();
    if (!load_graph_cache(path, GRAPH_FILE_KEY, vm, nm, *g))
        return fail(c, SMORE_EIO, std::string("cannot read a graph file (or other sampling methods): ") + path);
    c->g = g;
    c->hot_key.clear();
    c->semantics = SMORE_SEM_CPP;
    return upload_graph(c);
}

int smore_set_load_cache(smore_ctx* c, const char* dir) {
    if (!c) return SMORE_EINVAL;
    c->cache_dir = dir ? dir : "";
    return SMORE_OK;
}

int smore_last_load_info(const smore_ctx* c, double* seconds, int* threads, int* cache_hit) {
    if (!c) return SMORE_EINVAL;
    if (seconds) *seconds = c->load_seconds;
    if (threads) *threads = c->load_stats.threads;
    if (cache_hit) *cache_hit = c->load_stats.cache_hit;
    return SMORE_OK;
}

int smore_graph_info(const smore_ctx* c, int64_t* V, int64_t* E) {
    if (!c) return SMORE_EINVAL;
    if (V) *V = c->g->V;
    if (E) *E = c->g->E;
    return c->has_graph ? SMORE_OK : SMORE_ESTATE;
}

const char* smore_vertex_name(const smore_ctx* c, int64_t vid) {
    if (!c || vid < 0 || vid >= (int64_t)c->g->names.size()) return nullptr;
    return c->g->names[vid].c_str();
}

int smore_get_csr(const smore_ctx* c, int64_t* offsets, int32_t* targets) {
    if (!c || !c->has_graph) return SMORE_ESTATE;
    if (offsets) memcpy(offsets, c->g->offsets.data(), c->g->offsets.size() * sizeof(int64_t));
    if (targets) memcpy(targets, c->g->targets.data(), c->g->targets.size() * sizeof(int32_t));
    return SMORE_OK;
}

int smore_set_alias(smore_ctx* c, int which, const double* prob, const int64_t* alias, int64_t n) {
    if (!c || !prob || !alias) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    HostGraph& g = *c->g;
    int64_t want = which == SMORE_AT_CONTEXT ? g.E : g.V;
    if (which < 0 || which > 2 || n != want) return fail(c, SMORE_EINVAL, "alias table size mismatch");
    int64_t lim = g.V;
    for (int64_t i = 0; i < n; ++i) {
        if (alias[i] >= lim || alias[i] < -1 || !(prob[i] >= 0)) return fail(c, SMORE_EINVAL, "alias entry out of range");
        if (which != SMORE_AT_CONTEXT && alias[i] >= g.V) return fail(c, SMORE_EINVAL, "alias out of range");
    }
    hvec<double>& P = which == 0 ? g.vprob : which == 1 ? g.nprob : g.cprob;
    hvec<int64_t>& A = which == 0 ? g.valias : which == 1 ? g.nalias : g.calias;
    hvec<AliasEntry>& T = which == 0 ? g.vtab : which == 1 ? g.ntab : g.ctab;
    P.assign(prob, prob + n);
    A.assign(alias, alias + n);
    c->hot_key.clear();
    if (which == 0) c->field_src = -1;   // a new source law
    T.resize((size_t)n);
    alias_encode(P.data(), A.data(), n, which == SMORE_AT_CONTEXT ? g.targets.data() : nullptr, T.data());
    if (c->device < 0) return SMORE_OK;
    int rc;
    if ((rc = set_device(c))) return rc;
    AliasEntry*& d = which == 0 ? c->d_vtab : which == 1 ? c->d_ntab : c->d_ctab;
    c->packed_ok = false;
    if ((rc = upload(c, d, T.data(), T.size()))) return rc;
    return which == 0 && c->part_n > 1 ? apply_partition(c) : SMORE_OK;   // the new law, restricted again
}

int smore_get_alias(const smore_ctx* c, int which, double* prob, int64_t* alias, int64_t n) {
    if (!c || !c->has_graph || which < 0 || which > 2) return SMORE_EINVAL;
    const HostGraph& g = *c->g;
    const hvec<double>& P = which == 0 ? g.vprob : which == 1 ? g.nprob : g.cprob;
    const hvec<int64_t>& A = which == 0 ? g.valias : which == 1 ? g.nalias : g.calias;
    if (n != (int64_t)P.size()) return SMORE_EINVAL;
    if (prob) memcpy(prob, P.data(), n * sizeof(double));
    if (alias) memcpy(alias, A.data(), n * sizeof(int64_t));
    return SMORE_OK;
}

int smore_get_alias_encoded(const smore_ctx* c, int which, uint32_t* thresh, int32_t* alias, int64_t n) {
    if (!c || !c->has_graph || which < 0 || which > 2) return SMORE_EINVAL;
    const HostGraph& g = *c->g;
    const hvec<AliasEntry>& T = which == 0 ? g.vtab : which == 1 ? g.ntab : g.ctab;
    if (n != (int64_t)T.size()) return SMORE_EINVAL;
    for (int64_t i = 0; i < n; ++i) {
        if (thresh) thresh[i] = T[i].thresh;
        if (alias) alias[i] = T[i].alias;
    }
    return SMORE_OK;
}

// ---------------------------------------------------------------- tables
int smore_alloc_tables(smore_ctx* c, int dim, int ntables) {
    if (!c) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (dim <= 0 || dim > 512 || (ntables != 1 && ntables != 2 && ntables != 4))
        return fail(c, SMORE_EINVAL, "bad dim/ntables (1, 2, or 4: the CSE tables WU, WI, CU, CI)");
    int rc;
    if ((rc = set_device(c))) return rc;
    for (float*& t : c->d_table) dfree(t);
    c->dim = dim;
    c->dpad = (dim + 3) / 4 * 4;
    c->ntables = ntables;
    size_t bytes = (size_t)c->g->V * c->dpad * sizeof(float);
    // the C table of a two-table model carries HUB_SLOTS_MAX rows after V: the
    // block schedule's hub slots (blocks.cpp), never part of a rotating block
    c->c_slots = ntables == 2 ? std::min<int64_t>(HUB_SLOTS_MAX, c->g->V) : 0;
    const size_t cbytes = bytes + (size_t)c->c_slots * c->dpad * sizeof(float);
    // The embedding tables live in UNCACHED device memory: every row access is
    // served memory-side (Infinity Cache / HBM), which is coherent across the
    // 8 XCDs.  In the default coarse-grained memory each XCD's L2 keeps its own
    // copy of a row, so a plain-store (Hogwild) update made on one XCD is
    // overwritten by a read-modify-write from another XCD that still holds the
    // old line -- lost updates the reference's cache-coherent CPU Hogwild never
    // has (DESIGN.md "Scatter modes": DeepWalk held-out AUC on 2 blocks 0.82 ->
    // 0.87, the atomic level).  Measured on one box, C4 LINE-2 +2.5 %, C5
    // DeepWalk +8.6 %, C3 BPR equal (rows are random and miss L2 anyway).
    // SMORE_TABLE_MEM=coarse|finegrained|uncached overrides (experiments).
    unsigned flags = hipDeviceMallocUncached;
    if (const char* e = getenv("SMORE_TABLE_MEM")) {
        if (!strcmp(e, "coarse")) flags = hipDeviceMallocDefault;
        else if (!strcmp(e, "finegrained")) flags = hipDeviceMallocFinegrained;
        else if (!strcmp(e, "contiguous")) flags = hipDeviceMallocContiguous;
    }
    for (int t = 0; t < ntables; ++t)
        HIPCHK(c, hipExtMallocWithFlags((void**)&c->d_table[t], t == 1 ? cbytes : bytes, flags));
    for (int t = 0; t < ntables; ++t) HIPCHK(c, hipMemset(c->d_table[t], 0, t == 1 ? cbytes : bytes));
    c->blk.key.clear();   // the block tables' hub slots live in the new C table
    if (c->d_warp_stats) HIPCHK(c, hipMemset(c->d_warp_stats, 0, 2 * sizeof(unsigned long long)));
    if (c->d_hoprec_stats) HIPCHK(c, hipMemset(c->d_hoprec_stats, 0, 2 * sizeof(unsigned long long)));
    if (c->d_skewopt_stats) HIPCHK(c, hipMemset(c->d_skewopt_stats, 0, 2 * sizeof(unsigned long long)));
    if (c->d_cse_stats) HIPCHK(c, hipMemset(c->d_cse_stats, 0, 2 * sizeof(unsigned long long)));
    if (c->d_cbow_stats) HIPCHK(c, hipMemset(c->d_cbow_stats, 0, 2 * sizeof(unsigned long long)));
    if (c->d_eco_stats) HIPCHK(c, hipMemset(c->d_eco_stats, 0, 2 * sizeof(unsigned long long)));
    if (c->d_cbowdev_stats) HIPCHK(c, hipMemset(c->d_cbowdev_stats, 0, 2 * sizeof(unsigned long long)));
    return SMORE_OK;
}

int smore_init_table_glibc(smore_ctx* c, int which, uint64_t skip) {
    int rc;
    if ((rc = check_table(c, which))) return rc;
    GlibcRand r;
    r.discard(skip);
    std::vector<float> h((size_t)c->g->V * c->dpad, 0.0f);
    for (int64_t v = 0; v < c->g->V; ++v)
        for (int d = 0; d < c->dim; ++d)
            h[(size_t)v * c->dpad + d] = (float)((r.next() / (double)2147483647 - 0.5) / c->dim);
    if ((rc = set_device(c))) return rc;
    HIPCHK(c, hipMemcpy(c->d_table[which], h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return SMORE_OK;
}

int smore_init_table_glibc_offset(smore_ctx* c, int which, uint64_t skip, double offset) {
    int rc;
    if ((rc = check_table(c, which))) return rc;
    GlibcRand r;
    r.discard(skip);
    std::vector<float> h((size_t)c->g->V * c->dpad, 0.0f);
    for (int64_t v = 0; v < c->g->V; ++v)
        for (int d = 0; d < c->dim; ++d)
            h[(size_t)v * c->dpad + d] = (float)((r.next() / (double)2147483647 - 0.5) / c->dim + offset);
    if ((rc = set_device(c))) return rc;
    HIPCHK(c, hipMemcpy(c->d_table[which], h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return SMORE_OK;
}

int smore_init_table_uniform(smore_ctx* c, int which, uint64_t seed) {
    int rc;
    if ((rc = check_table(c, which))) return rc;
    if ((rc = set_device(c))) return rc;
    HIPCHK(c, launch_init_uniform(c->d_table[which], c->g->V, c->dim, c->dpad, seed, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SMORE_OK;
}

int smore_zero_table(smore_ctx* c, int which) {
    int rc;
    if ((rc = check_table(c, which))) return rc;
    if ((rc = set_device(c))) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_table[which], 0, (size_t)c->g->V * c->dpad * sizeof(float), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SMORE_OK;
}

int smore_set_table(smore_ctx* c, int which, const float* host, int64_t rows, int dim) {
    int rc;
    if ((rc = check_table(c, which))) return rc;
    if (!host || rows != c->g->V || dim != c->dim) return fail(c, SMORE_EINVAL, "table shape mismatch");
    if ((rc = set_device(c))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy2D(c->d_table[which], c->dpad * sizeof(float), host, dim * sizeof(float),
                          dim * sizeof(float), rows, hipMemcpyHostToDevice));
    return SMORE_OK;
}

int smore_get_table(const smore_ctx* cc, int which, float* host, int64_t rows, int dim) {
    smore_ctx* c = const_cast<smore_ctx*>(cc);
    int rc;
    if ((rc = check_table(c, which))) return rc;
    if (!host || rows != c->g->V || dim != c->dim) return fail(c, SMORE_EINVAL, "table shape mismatch");
    if ((rc = set_device(c))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy2D(host, dim * sizeof(float), c->d_table[which], c->dpad * sizeof(float),
                          dim * sizeof(float), rows, hipMemcpyDeviceToHost));
    return SMORE_OK;
}

int smore_table_device(smore_ctx* c, int which, void** dptr, int64_t* stride) {
    int rc;
    if ((rc = check_table(c, which))) return rc;
    if (dptr) *dptr = c->d_table[which];
    if (stride) *stride = c->dpad;
    return SMORE_OK;
}

int smore_set_semantics(smore_ctx* c, int semantics) {
    if (!c || (semantics != SMORE_SEM_CPP && semantics != SMORE_SEM_GO)) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (semantics == c->semantics) return SMORE_OK;
    c->packed_ok = false;
    c->field_src = -1;   // a new source law
    std::vector<double> tcum;
    if (semantics == SMORE_SEM_GO) build_go_tables(*c->g, tcum);
    else build_cpp_vn_tables(*c->g);
    c->go_unit_w = 1;
    for (int64_t e = 0; e < c->g->E && c->go_unit_w; ++e)
        if (c->g->weights[e] != 1.0) c->go_unit_w = 0;
    c->semantics = semantics;
    c->hot_key.clear();
    if (c->device < 0) return SMORE_OK;
    int rc;
    if ((rc = set_device(c))) return rc;
    if ((rc = upload(c, c->d_vtab, c->g->vtab.data(), c->g->vtab.size()))) return rc;
    if ((rc = upload(c, c->d_ntab, c->g->ntab.data(), c->g->ntab.size(), true))) return rc;
    if (semantics == SMORE_SEM_GO) {
        if ((rc = upload(c, c->d_tcum, tcum.data(), tcum.size()))) return rc;
    } else {
        dfree(c->d_tcum);
    }
    return c->part_n > 1 ? apply_partition(c) : SMORE_OK;   // the semantics' source law, restricted
}

int smore_skipped(smore_ctx* c, uint64_t* skipped) {
    if (!c || !skipped) return SMORE_EINVAL;
    int rc;
    if ((rc = set_device(c))) return rc;
    unsigned long long h = 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(&h, c->d_skipped, sizeof(h), hipMemcpyDeviceToHost));
    *skipped = h;
    return SMORE_OK;
}

// streaming-copy bandwidth of this GPU (membw.hip): two fresh buffers of
// `bytes`, one warm-up copy, then `reps` timed copies per variant (grid-
// stride default policy / non-temporal at 4 and 8 blocks per CU, one word per
// thread over the whole buffer); the best variant's (read +
// written bytes) / time.  Measurement only: nothing of the context changes.
int smore_copy_bandwidth(smore_ctx* c, uint64_t bytes, int reps, double* gbs) {
    if (!c || !gbs || reps < 1 || bytes < 4096) return SMORE_EINVAL;
    if (c->device < 0) return fail(c, SMORE_ESTATE, "host-only context");
    int rc;
    if ((rc = set_device(c))) return rc;
    const uint64_t n16 = bytes / 16;
    void *src = nullptr, *dst = nullptr;
    HIPCHK(c, hipMalloc(&src, n16 * 16));
    if (hipMalloc(&dst, n16 * 16) != hipSuccess) {
        (void)hipFree(src);
        return fail(c, SMORE_EHIP, "copy buffer allocation");
    }
    double best = 0.0;
    hipError_t e = hipMemsetAsync(src, 0x3c, n16 * 16, c->stream);
    for (int variant = 0; variant < 3 && e == hipSuccess; ++variant)
        for (int per_cu = 4; per_cu <= (variant == 2 ? 4 : 8) && e == hipSuccess; per_cu *= 2) {
            const int blocks = c->cus * per_cu;
            e = launch_copy(src, dst, n16, blocks, variant, c->stream);
            if (e == hipSuccess) e = hipEventRecord(c->ev0, c->stream);
            for (int r = 0; r < reps && e == hipSuccess; ++r) e = launch_copy(src, dst, n16, blocks, variant, c->stream);
            if (e == hipSuccess) e = hipEventRecord(c->ev1, c->stream);
            if (e == hipSuccess) e = hipEventSynchronize(c->ev1);
            float ms = 0.0f;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev0, c->ev1);
            if (e == hipSuccess && ms > 0) best = std::max(best, 2.0 * (double)n16 * 16 * reps / (ms * 1e-3) / 1e9);
        }
    (void)hipFree(src);
    (void)hipFree(dst);
    c->timed = false;
    if (e != hipSuccess) return fail(c, SMORE_EHIP, hipGetErrorString(e));
    *gbs = best;
    return SMORE_OK;
}

int smore_last_mode(const smore_ctx* c) { return c ? c->last_mode : -1; }

float smore_last_kernel_ms(const smore_ctx* c) {
    if (!c || !c->timed) return -1.0f;
    float ms = -1.0f;
    if (hipEventSynchronize(c->ev1) != hipSuccess) return -1.0f;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) return -1.0f;
    return ms;
}

int smore_deepwalk_order(int64_t V, int walk_times, uint64_t skip, int64_t* order) {
    if (V <= 0 || walk_times < 0 || !order) return SMORE_EINVAL;
    deepwalk_order(V, walk_times, skip, order);
    return SMORE_OK;
}

int smore_load_pretrain(smore_ctx* c, int which, const char* path) {
    int rc;
    if ((rc = check_table(c, which))) return rc;
    if (!path) return SMORE_EINVAL;
    if (c->g->names.empty()) return fail(c, SMORE_ESTATE, "warm start needs vertex names (load an edge list)");
    std::vector<float> h((size_t)c->g->V * c->dpad);
    if ((rc = set_device(c))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h.data(), c->d_table[which], h.size() * sizeof(float), hipMemcpyDeviceToHost));
    int64_t loaded = 0;
    if (!load_pretrain(path, *c->g, h.data(), c->dim, c->dpad, &loaded, c->err)) return SMORE_EIO;
    c->last_loaded = loaded;
    HIPCHK(c, hipMemcpy(c->d_table[which], h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return SMORE_OK;
}

int smore_save_weights(const smore_ctx* cc, int which, const char* path, int fmt) {
    smore_ctx* c = const_cast<smore_ctx*>(cc);
    int rc;
    if ((rc = check_table(c, which))) return rc;
    if (!path || fmt < 0 || fmt > 2) return fail(c, SMORE_EINVAL, "save_weights: bad path or format");
    std::vector<float> h((size_t)c->g->V * c->dpad);
    if ((rc = set_device(c))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h.data(), c->d_table[which], h.size() * sizeof(float), hipMemcpyDeviceToHost));
    if (!save_weights(path, *c->g, h.data(), c->g->V, c->dim, c->dpad, fmt, c->err)) return SMORE_EIO;
    return SMORE_OK;
}

// metapath2vec's typed neighbour index: NeighborsByType (pkg/hetero/
// hetero_graph.go:164-177) as every vertex's CSR targets stably grouped by the
// neighbour's type, with per-(vertex, type) offsets.
int smore_set_node_types(smore_ctx* c, const int32_t* node_type, int ntypes) {
    if (!c || !node_type || ntypes <= 0) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    const HostGraph& g = *c->g;
    const int64_t V = g.V, T = ntypes;
    for (int64_t v = 0; v < V; ++v)
        if (node_type[v] < 0 || node_type[v] >= ntypes) return fail(c, SMORE_EINVAL, "node type out of range");
    std::vector<int64_t> toff((size_t)(V * (T + 1)));
    std::vector<int32_t> tt((size_t)std::max<int64_t>(1, g.E));
    for (int64_t v = 0; v < V; ++v) {
        int64_t* o = toff.data() + v * (T + 1);
        const int64_t b = g.offsets[v], e = g.offsets[v + 1];
        std::vector<int64_t> cnt((size_t)T, 0);
        for (int64_t x = b; x < e; ++x) cnt[node_type[g.targets[x]]]++;
        o[0] = b;
        for (int64_t t = 0; t < T; ++t) o[t + 1] = o[t] + cnt[t];
        std::vector<int64_t> pos(o, o + T);
        for (int64_t x = b; x < e; ++x) {
            const int32_t n = g.targets[x];
            tt[pos[node_type[n]]++] = n;
        }
    }
    int rc;
    if ((rc = set_device(c))) return rc;
    if ((rc = upload(c, c->d_ntype, node_type, (size_t)V))) return rc;
    if ((rc = upload(c, c->d_toff, toff.data(), toff.size()))) return rc;
    if ((rc = upload(c, c->d_ttargets, tt.data(), tt.size()))) return rc;
    c->ntypes = ntypes;
    return SMORE_OK;
}

// CTDNE's temporal graph (pkg/temporal/temporal_graph.go:60-170, 254-288):
// OutEdges per source sorted by timestamp (stable: Go's sort.Slice leaves the
// order of equal timestamps unspecified), the active time range of every
// vertex over its out- and in-edges ({0, 0} without edges), Min/MaxTime.
int smore_set_temporal_edges(smore_ctx* c, int64_t E, const int32_t* src, const int32_t* dst, const double* ts) {
    if (!c || E < 0 || (E > 0 && (!src || !dst || !ts))) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    const int64_t V = c->g->V;
    for (int64_t i = 0; i < E; ++i)
        if (src[i] < 0 || src[i] >= V || dst[i] < 0 || dst[i] >= V)
            return fail(c, SMORE_EINVAL, "temporal edge id out of range");
    std::vector<int64_t> off((size_t)V + 1, 0);
    for (int64_t i = 0; i < E; ++i) off[(size_t)src[i] + 1]++;
    for (int64_t v = 0; v < V; ++v) off[v + 1] += off[v];
    std::vector<int64_t> slot(off.begin(), off.end() - 1), perm((size_t)std::max<int64_t>(1, E));
    for (int64_t i = 0; i < E; ++i) perm[slot[src[i]]++] = i;
    std::vector<int32_t> tgt((size_t)std::max<int64_t>(1, E));
    std::vector<double> tts((size_t)std::max<int64_t>(1, E));
    std::vector<double> tmin((size_t)V, std::numeric_limits<double>::max());
    std::vector<double> tmax((size_t)V, -std::numeric_limits<double>::max());
    double lo = std::numeric_limits<double>::max(), hi = -std::numeric_limits<double>::max();
    for (int64_t v = 0; v < V; ++v) {
        std::stable_sort(perm.begin() + off[v], perm.begin() + off[v + 1],
                         [&](int64_t a, int64_t b) { return ts[a] < ts[b]; });
        for (int64_t x = off[v]; x < off[v + 1]; ++x) {
            tgt[x] = dst[perm[x]];
            tts[x] = ts[perm[x]];
        }
    }
    for (int64_t i = 0; i < E; ++i) {
        for (int32_t v : {src[i], dst[i]}) {
            tmin[v] = std::min(tmin[v], ts[i]);
            tmax[v] = std::max(tmax[v], ts[i]);
        }
        lo = std::min(lo, ts[i]);
        hi = std::max(hi, ts[i]);
    }
    for (int64_t v = 0; v < V; ++v)
        if (tmin[v] == std::numeric_limits<double>::max()) tmin[v] = tmax[v] = 0.0;
    int rc;
    if ((rc = set_device(c))) return rc;
    if ((rc = upload(c, c->d_t_off, off.data(), off.size()))) return rc;
    if ((rc = upload(c, c->d_t_tgt, tgt.data(), tgt.size()))) return rc;
    if ((rc = upload(c, c->d_t_ts, tts.data(), tts.size()))) return rc;
    if ((rc = upload(c, c->d_t_min, tmin.data(), tmin.size()))) return rc;
    if ((rc = upload(c, c->d_t_max, tmax.data(), tmax.size()))) return rc;
    c->t_min_time = lo;
    c->t_max_time = hi;
    c->has_temporal = true;
    return SMORE_OK;
}

// ---------------------------------------------------------------- row census
int smore_census_begin(smore_ctx* c) {
    if (!c) return SMORE_EINVAL;
    if (int rc_ = refuse_cse(c)) return rc_;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    int rc;
    if ((rc = set_device(c))) return rc;
    const size_t V = (size_t)std::max<int64_t>(1, c->g->V);
    for (auto*& p : c->d_census) {
        if (!p) HIPCHK(c, hipMalloc((void**)&p, V * sizeof(unsigned long long)));
        HIPCHK(c, hipMemsetAsync(p, 0, V * sizeof(unsigned long long), c->stream));
    }
    c->census = true;
    c->census_ok = false;
    return SMORE_OK;
}

int smore_census_end(smore_ctx* c, double units) {
    if (!c) return SMORE_EINVAL;
    if (!c->census) return fail(c, SMORE_ESTATE, "no census in progress (smore_census_begin)");
    c->census = false;
    if (!(units > 0.0)) return fail(c, SMORE_EINVAL, "census: units must be > 0");
    int rc;
    if ((rc = set_device(c))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t V = (size_t)c->g->V;
    std::vector<unsigned long long> h(V);
    for (int t = 0; t < 2; ++t) {
        if (V) HIPCHK(c, hipMemcpy(h.data(), c->d_census[t], V * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        c->census_rate[t].resize(V);
        for (size_t i = 0; i < V; ++i) c->census_rate[t][i] = (double)h[i] / units;
    }
    c->census_ok = true;
    c->census_gen++;
    return SMORE_OK;
}

// ---------------------------------------------------------------- walk partition
int smore_set_walk_owner(smore_ctx* c, int64_t lo, int64_t hi) {
    if (!c) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (hi < 0) {
        c->own_lo = 0;
        c->own_hi = -1;
        return SMORE_OK;
    }
    if (lo < 0 || lo > hi || hi > c->g->V) return fail(c, SMORE_EINVAL, "walk owner range outside [0, V]");
    c->own_lo = lo;
    c->own_hi = hi;
    return SMORE_OK;
}

int smore_walk_parts(smore_ctx* c, int nparts, int64_t* bounds) {
    if (!c || !bounds || nparts < 1) return SMORE_EINVAL;
    if (!c->has_graph) return fail(c, SMORE_ESTATE, "no graph");
    if (nparts > c->g->V) return fail(c, SMORE_EINVAL, "more parts than vertices");
    if (!c->census_ok) return fail(c, SMORE_ESTATE, "walk parts need a row census (smore_census_begin / _end)");
    std::vector<int64_t> bound;
    source_bounds(c->census_rate[0], nparts, bound);
    std::copy(bound.begin(), bound.end(), bounds);
    return SMORE_OK;
}

// ---------------------------------------------------------------- replica exchange
static int delta_args(smore_ctx* c, const void* T, const void* S, const void* D, const void* R, int64_t n) {
    if (!c || !T || !S || !D || !R || n < 0 || (n & 3)) return fail(c, SMORE_EINVAL, "delta: bad buffers");
    for (const void* p : {T, S, D, R})
        if ((uintptr_t)p & 15) return fail(c, SMORE_EINVAL, "delta: buffers must be 16-byte aligned");
    return set_device(c);
}

int smore_delta_begin(smore_ctx* c, const void* T, void* S, void* D, void* R, int64_t n) {
    int rc;
    if ((rc = delta_args(c, T, S, D, R, n))) return rc;
    HIPCHK(c, launch_delta_begin((const float*)T, (float*)S, (float*)D, (float*)R, (uint64_t)n, c->cus, c->stream));
    return SMORE_OK;
}

int smore_delta_end(smore_ctx* c, void* T, void* S, const void* D, const void* R, float scale, int64_t n) {
    int rc;
    if ((rc = delta_args(c, T, S, D, R, n))) return rc;
    HIPCHK(c, launch_delta_end((float*)T, (float*)S, (const float*)D, (const float*)R, scale, (uint64_t)n, c->cus,
                               c->stream));
    return SMORE_OK;
}

int smore_delta_cycle(smore_ctx* c, void* T, void* S, void* D, void* R, float scale, int64_t n) {
    int rc;
    if ((rc = delta_args(c, T, S, D, R, n))) return rc;
    HIPCHK(c, launch_delta_cycle((float*)T, (float*)S, (float*)D, (float*)R, scale, (uint64_t)n, c->cus, c->stream));
    return SMORE_OK;
}

static int delta_rows_args(smore_ctx* c, const void* T, const void* S, const void* D, const void* R,
                           const void* scale, int64_t rows, int64_t stride) {
    if (!c || !scale || rows < 0 || stride <= 0 || (stride & 3) || stride > (1 << 20))
        return fail(c, SMORE_EINVAL, "delta rows: bad shape");
    if ((uintptr_t)scale & 3) return fail(c, SMORE_EINVAL, "delta rows: scale must be 4-byte aligned");
    return delta_args(c, T, S, D, R, rows * stride);
}

int smore_delta_end_rows(smore_ctx* c, void* T, void* S, const void* D, const void* R, const void* scale,
                         int64_t rows, int64_t stride) {
    int rc;
    if ((rc = delta_rows_args(c, T, S, D, R, scale, rows, stride))) return rc;
    HIPCHK(c, launch_delta_end_rows((float*)T, (float*)S, (const float*)D, (const float*)R, (const float*)scale,
                                    (uint64_t)rows, (int)stride, c->cus, c->stream));
    return SMORE_OK;
}

int smore_delta_cycle_rows(smore_ctx* c, void* T, void* S, void* D, void* R, const void* scale, int64_t rows,
                           int64_t stride) {
    int rc;
    if ((rc = delta_rows_args(c, T, S, D, R, scale, rows, stride))) return rc;
    HIPCHK(c, launch_delta_cycle_rows((float*)T, (float*)S, (float*)D, (float*)R, (const float*)scale,
                                      (uint64_t)rows, (int)stride, c->cus, c->stream));
    return SMORE_OK;
}

}  // extern "C"

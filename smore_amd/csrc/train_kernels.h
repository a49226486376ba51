// train_kernels.h -- launch interface of the gfx950 hot-path kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "../../include/smore_hip.h"
#include "device_common.h"

namespace smore {

// scatter of an update-kernel instantiation (template parameter MODE); a
// SMORE_SERIAL call runs the MODE_STORE instantiation with one sample group
enum { MODE_STORE = SMORE_HOGWILD, MODE_ATOMIC = SMORE_ATOMIC, MODE_HYBRID = SMORE_HYBRID };

struct EdgeArgs {
    DevGraph g;
    const float* sig;              // 1001-entry fastSigmoid table
    float* W;                      // [V][dpad]
    float* C;                      // [V][dpad] (== W for shared-table models)
    unsigned long long* skipped;   // samples whose source had no out-edge
    const double* tcum;            // Go semantics: per-vertex prefix sums of edge weights
    // hybrid write-combining of the super-hot context rows (edge kernel only):
    // open-addressing hash {id, slot} (SH_HASH entries, id -1 = empty), the
    // slot -> id list, sh_rows slots (0 = off), a block flush every sh_flush rounds
    const int2* sh_hash;
    const int32_t* sh_ids;
    int sh_rows, sh_flush;
    int sh_flush_w;                // W-key slots (SMORE_SH_WROWS) drained every sh_flush_w rounds too (0: off)
    // per-slot drain intervals: every slot drains every sh_flush rounds (a
    // power of two); slot i also every 2^j rounds when i < sh_lvl[j] (the slot
    // list is sorted by rate, so the slots due at a round are a prefix;
    // all-zero sh_lvl: one interval for all)
    int sh_lvl[8];
    // edge kernels: the pre-drawn sample records of samples [begin, begin+count)
    // (draw_kernel), rec_width(KMAX) int32 each
    const int32_t* rec;
    const uint64_t* count_dev;     // non-null: the record count is read here (device-side pair totals)
    const uint64_t* rec_base;      // non-null: the launch's records are [*rec_base, *count_dev) (block buckets)
    unsigned long long* work;      // Hogwild edge kernels: chunk counter, zeroed per launch
    int alpha_rec;                 // learning rate in record word 2 + KMAX: 1 walk pairs (pair kernels),
                                   // 2 independent samples (the edge kernel: the hot/cold split)
    uint32_t pair_slice;           // pair kernels: records per group slice (0: CH_ROUNDS)
    // negative-gradient weight (2-D block schedule): a cell
    // draws its negatives from its C block's restricted law, but gets samples
    // in proportion to the block's CONTEXT mass; weighting the negatives'
    // step by NegativeSample's block mass over the cell's share restores the
    // epoch's negative law.  neg_scale <= 0: 1 (off).  neg_lo / neg_hi
    // non-null (walk cells): neg_scale is the block's negative share and the
    // weight is computed on the device from the round's record counts,
    // neg_scale * (*neg_hi - *neg_lo) / records.
    float neg_scale;
    const uint64_t* neg_lo;
    const uint64_t* neg_hi;
    // pair kernel, hybrid: a run's W row is STORED when it is not hot-tagged
    // (the edge rule), instead of adding its delta atomically (walk cells of
    // the block schedule: their runs are ~1 record long)
    int w_plain;
    // a block bucket's launch in parts: records [lo, hi) of the bucket's
    // range with lo = n part_q / part_n (part_n <= 1: the whole bucket)
    uint32_t part_q, part_n;
    // walk records through the (row-prefetching) edge kernel instead of the
    // pair kernel (block walk cells: their W runs are ~1 record long)
    int rec_edge;
    int w_comb;          // pair kernel (walk cells): the runs' W rows looked up in the write-combined set
    uint64_t begin, count, total, seed;
    double alpha0;
    float reg;
    int dpad, K, model, mode;
};

// DeepWalk: a chunk of walks [walk_begin, walk_begin + nwalks)
struct WalkArgs {
    const int64_t* order;          // walk start vertices of walks [order_base, ...) (a slice of the full order)
    uint64_t order_base;
    int32_t* walks;                // nwalks x (steps + 1); C++ walks hold id | hc << 30 | hw << 31
    int32_t* lens;                 // nwalks
    uint64_t walk_begin, nwalks, total_walks;
    int steps, window;
    int rule;                      // pair rule: 0 DeepWalk SkipGrams (random shrink), 1 Walklets ScaleSkipGrams
    int window_min;                // Walklets: pairs at distance [window_min, window] (clamped as the reference)
    // node2vec (Go, rule 2): 1/p, 1/q, raw CSR edge weights and a per-vertex
    // sorted copy of the CSR targets (areNeighbors by binary search)
    double inv_p, inv_q;
    const double* wts;
    const int32_t* nbr_sorted;
    // metapath2vec (Go, rule 3): node types, every vertex's CSR targets grouped
    // by type (push order kept) with offsets toff[v * (ntypes + 1) + t], the
    // meta-paths (type ids, path p = paths[path_off[p] .. path_off[p + 1]))
    const int32_t* ntype;
    const int32_t* ttargets;
    const int64_t* toff;
    const int32_t* paths;
    const int32_t* path_off;
    int ntypes, npaths;
    int slot_extra;                // draws before the step draws (metapath2vec: the path choice)
    // walk partition (smore_set_walk_owner): only pairs whose center (W row)
    // walk[i] is in [own_lo, own_hi) become records; every pair still takes
    // its draws, so the records are the one-context records restricted
    int32_t own_lo = 0, own_hi = 0x7FFFFFFF;
};

// APP: units [unit_begin, unit_begin + n) of walk_times * V * sample_times; unit
// u = w * sample_times + s jumps from order[w - order_base] (APP::Train)
struct AppArgs {
    const int64_t* order;
    uint64_t order_base, unit_begin, n, total_walks;
    int sample_times;
    double jump;
};

// lanes per sample group: G = min(64, pow2ceil(dpad / 4)); lane l owns the
// row's 16-B chunks l, l+G, ... in M = regs_of(dpad) registers
// (device_common.h elem_off; DESIGN.md "Arithmetic spec")
int lanes_of(int dpad);
inline int regs_of(int dpad) {
    const int G = lanes_of(dpad);
    return 4 * ((dpad / 4 + G - 1) / G);
}
// int32 words per pre-drawn edge-sample record {v, c, n_1..n_K, pad}: the
// smallest power of two >= 2 + KMAX, at least 4 (whole 16-B words)
constexpr int rec_width(int kmax) {
    int r = 4;
    while (r < 2 + kmax) r <<= 1;
    return r;
}
constexpr uint64_t CH_ROUNDS = 128;   // rounds per dynamically handed-out chunk
inline int kmax_of(int K) { return K <= 5 ? 5 : K <= 10 ? 10 : 20; }
hipError_t launch_delta_begin(const float* T, float* S, float* D, float* R, uint64_t n, int cus, hipStream_t st);
hipError_t launch_delta_end(float* T, float* S, const float* D, const float* R, float scale, uint64_t n, int cus,
                            hipStream_t st);
hipError_t launch_delta_cycle(float* T, float* S, float* D, float* R, float scale, uint64_t n, int cus,
                              hipStream_t st);
hipError_t launch_pair_count(const WalkArgs& w, uint64_t seed, uint32_t* count, hipStream_t st);
// upper bound on the skip-gram pairs of one walk of `steps` steps: DeepWalk
// (window shrink >= 1) or Walklets (two clamped ranges of window - window_min + 1)
inline uint64_t pair_bound(int steps, int window, int rule = 0, int window_min = 0) {
    const uint64_t L = (uint64_t)steps + 1;
    if (rule == 1) return L * 2 * (uint64_t)std::max(1, window - window_min + 1);
    const uint64_t r = std::min<uint64_t>(2 * (uint64_t)window, L - 1);
    return L * r;
}
hipError_t scan_pair_counts(const uint32_t* count, uint64_t* off, uint64_t n, void** temp, size_t* temp_bytes,
                            hipStream_t st);
hipError_t launch_pair_emit(const DevGraph& g, const WalkArgs& w, uint64_t seed, int K, double alpha0,
                            const uint64_t* off, int32_t* rec, hipStream_t st);
hipError_t launch_pack(const DevGraph& g, uint64_t E, uint4* vt32, uint4* ct16, hipStream_t st);
// draw_split_kernel (train_draw.hip): the draws with the rate in the record,
// hot records from the front, the others from the back; counts[0] / [1] the
// hot / cold records (zeroed by the caller)
hipError_t launch_draw_split(const DevGraph& g, uint64_t seed, uint64_t begin, uint64_t count, int K, double alpha0,
                             uint64_t total, int base, int32_t* rec, unsigned long long* skipped,
                             unsigned long long* counts, hipStream_t st);
hipError_t launch_draw(const DevGraph& g, uint64_t seed, uint64_t begin, uint64_t count, int K, int32_t* rec,
                       unsigned long long* skipped, hipStream_t st);
constexpr int SH_HASH = 256;   // entries of the super-hot row hash (power of two, > the rows)
constexpr int32_t SH_WKEY = 1 << 30;   // write-combine key bit: a W row of a two-table model
// dynamic LDS of the hybrid edge kernel: hash, slot ids, pending deltas
// write-combined rows that fit the LDS budget: SMORE_SH_LDS floats of pending
// deltas (default 8192: 32 KB, three 256-thread blocks per CU with the hash,
// ids and sigmoid table), below the hash's size.  160 rows at d=64 (40 KB,
// hash 512) measured slower at one GPU (84.1 vs 83.6 ms per 2^27, C4) and in
// the block schedule's cells (C4, 8 GPUs: 5.44 vs 5.76 x predicted)
inline int sh_rows_max(int dpad) {
    static const int lds = [] {
        const char* e = getenv("SMORE_SH_LDS");
        const int v = e ? atoi(e) : 8192;
        return v > 0 ? v : 8192;
    }();
    const int r = lds / (dpad > 0 ? dpad : 1);
    return r < SH_HASH - 1 ? r : SH_HASH - 1;
}

inline size_t sh_lds_bytes(int sh_rows, int dpad) {
    return sh_rows > 0 ? SH_HASH * 8 + (size_t)sh_rows * 4 + (size_t)sh_rows * dpad * 4 : 0;
}
inline uint32_t sh_hash_of(int32_t id) { return ((uint32_t)id * 2654435761u) >> 24; }
// Go edge models on records: go_draw_kernel (train_go.hip; unit_w: every edge
// weight is 1) then go_rec_kernel (go_rec.h; UpdateFamily::GoRec)
hipError_t launch_go_draw(const DevGraph& g, const double* tcum, int unit_w, uint64_t seed, uint64_t begin,
                          uint64_t count, int K, int32_t* rec, unsigned long long* skipped, hipStream_t st);
hipError_t launch_go_walk(const EdgeArgs& a, const WalkArgs& w, int grid, hipStream_t st);
hipError_t launch_go_sample(const DevGraph& g, const double* tcum, uint64_t seed, uint64_t begin, uint64_t count,
                            int K, int32_t* out, hipStream_t st);
hipError_t launch_walk_gen(const DevGraph& g, const WalkArgs& w, uint64_t seed, hipStream_t st);
// HPE: samples [begin, begin + n) of total (HPE::Train), walk_steps community
// steps each
struct HpeArgs {
    uint64_t begin, n, total;
    int walk_steps;
};
hipError_t launch_hpe_records(const DevGraph& g, const HpeArgs& p, uint64_t seed, int K, double alpha0, int32_t* rec,
                              unsigned long long* skipped, hipStream_t st);
hipError_t launch_app_records(const DevGraph& g, const AppArgs& p, uint64_t seed, int K, double alpha0, int32_t* rec,
                              hipStream_t st);
constexpr int APP_MAX_STEPS = 1 << 24;   // jumping-walk bound (oracle APP_MAX_STEPS)
// caller-supplied pairs (smore_train_pairs): pairs per RNG unit (oracle ORC_PAIR_BLOCK)
constexpr uint64_t PAIR_BLOCK = (uint64_t)1 << 20;
hipError_t launch_caller_pairs(const DevGraph& g, const int32_t* pv, const int32_t* pc, uint64_t n, uint64_t first,
                               int K, float alpha, uint64_t seed, uint64_t unit0, int go, int tagged, int32_t* rec,
                               hipStream_t st);
// row census (smore_census_begin): per record +1 at W[word 0] and at C[word 1]
// and C[each negative >= 0]; records whose word 1 is negative (HPE's skipped
// samples and finished walks) count nothing.  count_dev: the count on the device
hipError_t launch_row_census(const int32_t* rec, uint64_t n, const uint64_t* count_dev, int RW, int K,
                             unsigned long long* cw, unsigned long long* cc, int cus, hipStream_t st);
// WARP (warp_kernels.h; train_warp_<s|a>.hip): the update kernel draws the
// negatives of trials 1..31 itself
constexpr int WARP_TRIALS = 32;              // src/proNet.cpp:1366
constexpr int WARP_KMAX = 5;                 // record width of the K = 1 draw
enum { WARP_STORE = MODE_STORE, WARP_ATOMIC = MODE_ATOMIC };

struct WarpArgs {
    DevGraph g;
    const float* sig;              // 1001-entry fastSigmoid table
    float* T;                      // [V][dpad], the one table
    const int32_t* rec;            // {v, i, j0, -1 ..} per sample, rec_width(WARP_KMAX) words (tagged ids)
    unsigned long long* work;      // chunk counter, zeroed per launch
    unsigned long long* stats;     // {trials executed, samples that updated}, accumulated
    uint64_t begin, count, total, seed;
    double alpha0;
    int dpad, mode;                // mode: SMORE_* scatter (2 = serial)
    int groups;                    // sample groups of a block that take samples (<= 256 / G; the rest idle)
};

// HOP-REC (hoprec_kernels.h; train_hoprec_<s|a>.hip): a sample is walk_steps
// ranking steps on {v, i_w, j_w0..j_w4}, every id pre-drawn by
// hoprec_draw_kernel (train_hoprec_draw.hip) from the sample's Philox unit
constexpr int HOPREC_NEG = 5;                // negatives per step (src/proNet.cpp:1472)
constexpr int HOPREC_MAX_STEPS = 10;         // walk_steps accepted
constexpr int HOPREC_KMAX = 5;               // the family's one instantiation bucket
constexpr uint32_t HOPREC_ATTEMPTS = 1u << 16;   // a rejection loop gives up after this many draws
// int32 words of a record {v, then per step i_w, j_w0..j_w4}: padded to whole 16-B words
constexpr int hoprec_width(int steps) { return (1 + (1 + HOPREC_NEG) * steps + 3) & ~3; }

struct HopRecArgs {
    const float* sig;              // 1001-entry fastSigmoid table
    float* T;                      // [V][dpad], the one table
    const int32_t* rec;            // hoprec_width(steps) words per sample (tagged ids; -1 from the step a sample stopped at)
    unsigned long long* work;      // chunk counter, zeroed per launch
    unsigned long long* stats;     // {gates tested, gates passed}, accumulated
    uint64_t begin, count, total;
    double alpha0;
    int dpad, mode;                // mode: SMORE_* scatter (2 = serial)
    int steps;                     // walk_steps
};
// the draws of samples [begin, begin + count): records, and (slots non-null) the
// Philox slots each sample consumed; a sample that stopped early is counted in *skipped
hipError_t launch_hoprec_draw(const DevGraph& g, const int32_t* field, uint64_t seed, uint64_t begin, uint64_t count,
                              int steps, int32_t* rec, uint32_t* slots, unsigned long long* skipped, hipStream_t st);

// Skew-OPT (skewopt_kernels.h; train_skewopt_<s|a>.hip): one positive pair and
// sixteen negatives per sample, every id pre-drawn by launch_draw with K = 16
constexpr int SKEW_NEG = 16;                 // negatives per sample (src/proNet.cpp:1532)
constexpr int SKEWOPT_KMAX = 20;             // record width of the K = 16 draw: rec_width(20) = 32 words

struct SkewOptArgs {
    const float* sig;              // 1001-entry fastSigmoid table
    float* T;                      // [V][dpad], the one table
    const int32_t* rec;            // {v, i, j_0..j_15, -1 ..} per sample, rec_width(SKEWOPT_KMAX) words (tagged ids)
    unsigned long long* work;      // chunk counter, zeroed per launch
    unsigned long long* stats;     // {gates passed, samples that updated}, accumulated
    uint64_t begin, count, total;
    double alpha0;
    float xi, omega;               // the rule's margin and scale, rounded to fp32 once
    int eta;                       // the power (>= 1)
    int dpad, mode;                // mode: SMORE_* scatter (2 = serial)
};

// CSE (cse_kernels.h; train_cse_<s|a>.hip): nemf (rank 0) and nerank (rank 1) train four
// tables WU, WI, CU, CI; a sample is two neighbourhood passes of walk_steps
// steps (A: vertex WI[c], contexts CI; B: vertex WU[v], contexts CU) and a
// direct term on WU[v], WI[c] and 5 (nemf) or 16 (nerank) negative WI rows,
// every id pre-drawn by cse_draw_kernel (train_cse_draw.hip)
constexpr int CSE_NEG = 5;                   // negatives per pass step and of nemf's direct term (NEMF.cpp:108)
constexpr int CSE_RANK_NEG = 16;             // nerank's direct negatives (src/proNet.cpp:2632)
constexpr int CSE_MAX_STEPS = 10;            // walk_steps accepted
constexpr uint32_t CSE_ATTEMPTS = 1u << 16;  // a rejection loop gives up after this many draws
constexpr int cse_dneg(int rank) { return rank ? CSE_RANK_NEG : CSE_NEG; }
// int32 words of a record {v, c, A: n_00..n_04, then per step s >= 1 ctx_s, n_s0..n_s4; B: the
// same; the direct negatives}: 12 steps + 5 or 16, padded to whole 16-B words (plain ids, -1: none)
constexpr int cse_width(int steps, int rank) { return (12 * steps + cse_dneg(rank) + 3) & ~3; }

struct CseArgs {
    const float* sig;              // 1001-entry fastSigmoid table
    float* T[4];                   // WU, WI, CU, CI, [V][dpad] each
    const int32_t* rec;            // cse_width(steps, rank) words per sample
    unsigned long long* work;      // chunk counter, zeroed per launch
    unsigned long long* stats;     // nerank {gates tested, updates made}, accumulated
    uint64_t begin, count, total;
    double alpha0;
    int dpad, mode;                // mode: SMORE_* scatter (2 = serial)
    int steps, rank;               // walk_steps; 0 nemf, 1 nerank
};
// the draws of samples [begin, begin + count): records, and (slots non-null) the Philox slots each
// sample consumed; a sample without a target, or one of whose walks or rejection loops stopped
// early, is counted once in *skipped
hipError_t launch_cse_draw(const DevGraph& g, const int32_t* field, uint64_t seed, uint64_t begin, uint64_t count,
                           int steps, int rank, int32_t* rec, uint32_t* slots, unsigned long long* skipped,
                           hipStream_t st);

// CBOW, the set-sum rule of GCN (SMORE_CBOW_GCN) and TEXTGCN (SMORE_CBOW_TEXTGCN) (cbow_kernels.h;
// train_cbow_<s|a>.hip): a sample scores the sum of its w-set rows against the sum of its c-set
// rows (label 1) and of K uniform field-1 sets (label 0), every set of S rows of table 0 takes
// one shared delta, every id pre-drawn by cbow_draw_kernel (train_cbow_draw.hip)
constexpr int CBOW_MAX_S = 10;                // walk_steps accepted
constexpr int CBOW_MAX_K = 20;                // negative_samples accepted
constexpr int CBOW_BATCH = 5;                 // rows of a set gathered together (the kernels' KMAX)
constexpr uint32_t CBOW_ATTEMPTS = 1u << 16;  // a rejection loop gives up after this many draws
// int32 words of a record {vertex, context, c-set[S], w-set[S], K x neg-set[S]}, padded to whole
// 16-B words (plain ids; an empty set is S times -1, a skipped sample all -1)
constexpr int cbow_width(int S, int K) { return (2 + 2 * S + K * S + 3) & ~3; }

struct CbowArgs {
    const float* sig;              // 1001-entry fastSigmoid table
    float* T;                      // w_vertex, [V][dpad]
    const int32_t* rec;            // cbow_width(S, K) words per sample
    const uint8_t* clean;          // per sample: 1 when the c-set and negative ids are pairwise distinct
    unsigned long long* work;      // chunk counter, zeroed per launch
    unsigned long long* stats;     // {clean samples, ordered samples}, accumulated
    uint64_t begin, count, total;
    double alpha0;
    float reg;
    int dpad, mode;                // mode: SMORE_* scatter (2 = serial)
    int S, K;                      // walk_steps, negative_samples
};
// the draws of samples [begin, begin + count): records, the clean flags, and (slots non-null)
// the Philox slots each sample consumed; a skipped sample is counted once in *skipped
hipError_t launch_cbow_draw(const DevGraph& g, const int32_t* field, uint64_t seed, uint64_t begin, uint64_t count,
                            int model, int S, int K, int32_t* rec, uint8_t* clean, uint32_t* slots,
                            unsigned long long* skipped, hipStream_t st);

// ECO, the sampled-softmax choice rule (eco_kernels.h; train_eco_<s|a>.hip): a sample is ECO_LISTS
// lists {c1, c2, n_0..n_{K-1}} around one vertex v, all rows of table 0; a list's rows move by the
// softmax of their scores over the list, W[v] takes the lists' summed delta last; every id
// pre-drawn by eco_draw_kernel (train_eco_draw.hip)
constexpr int ECO_LISTS = 5;                 // lists per sample (src/proNet.cpp:2239)
constexpr int ECO_MAX_K = 20;                // negative_samples accepted
constexpr int ECO_BATCH = 5;                 // negative rows gathered together
constexpr uint32_t ECO_ATTEMPTS = 1u << 16;  // the source loop gives up after this many draws
// int32 words of a record {v, then per list c1, c2, n_0..n_{K-1}}, padded to whole 16-B words
// (plain ids; a skipped sample all -1)
constexpr int eco_width(int K) { return (1 + ECO_LISTS * (2 + K) + 3) & ~3; }

struct EcoArgs {
    float* T;                      // w_vertex, [V][dpad]
    const int32_t* rec;            // eco_width(K) words per sample
    const uint8_t* clean;          // per sample: bit 0 all its 1 + 5 (2 + K) ids are pairwise distinct, bit 1 + l: v and list l's are
    unsigned long long* work;      // chunk counter, zeroed per launch
    unsigned long long* stats;     // {clean samples, ordered samples}, accumulated
    uint64_t begin, count, total;
    double alpha0;
    float reg;
    int dpad, mode;                // mode: SMORE_* scatter (2 = serial)
    int K;                         // negative_samples
};
// the draws of samples [begin, begin + count): records, the clean flags, and (slots non-null)
// the Philox slots each sample consumed; a skipped sample is counted once in *skipped
hipError_t launch_eco_draw(const DevGraph& g, const int32_t* field, uint64_t seed, uint64_t begin, uint64_t count,
                           int K, int32_t* rec, uint8_t* clean, uint32_t* slots, unsigned long long* skipped,
                           hipStream_t st);

// CBOWdev, the bag-of-words event rule of TEXTGCNdev (cbowdev_kernels.h; train_cbowdev_<s|a>.hip):
// a sample sums num_events x num_words rows of table 1 (w_context) into a bag, steps W[event]
// and ten uniform field-1 rows of table 0 per iteration against the bag and against W[user], one
// row at a time and in place, then W[user] and every bag row take their accumulated deltas; every
// id pre-drawn by cbowdev_draw_kernel (train_cbowdev_draw.hip)
constexpr int CBOWDEV_MAX = 10;                  // num_events and num_words accepted
constexpr int CBOWDEV_NEG = 5;                   // negative pairs per iteration (the reference's constant)
constexpr int CBOWDEV_BATCH = 5;                 // bag rows gathered together (the kernels' KMAX)
constexpr uint32_t CBOWDEV_ATTEMPTS = 1u << 16;  // a rejection loop gives up after this many draws
// int32 words of a record {user, event, bag[E N], E x {a0, b0, .. a4, b4}}, padded to whole 16-B
// words (plain ids; a skipped sample all -1)
constexpr int cbowdev_width(int E, int N) { return (2 + E * N + 2 * CBOWDEV_NEG * E + 3) & ~3; }

struct CbowDevArgs {
    const float* sig;              // 1001-entry fastSigmoid table
    float* T;                      // w_vertex, [V][dpad]
    float* C;                      // w_context, [V][dpad]
    const int32_t* rec;            // cbowdev_width(E, N) words per sample
    const uint8_t* clean;          // per sample: 1 when user, event and the negative ids are pairwise distinct
    unsigned long long* work;      // chunk counter, zeroed per launch
    unsigned long long* stats;     // {clean samples, ordered samples}, accumulated
    uint64_t begin, count, total;
    double alpha0;
    float reg;
    int dpad, mode;                // mode: SMORE_* scatter (2 = serial)
    int E, N;                      // num_events, num_words
};
// the draws of samples [begin, begin + count): records, the clean flags, and (slots non-null)
// the Philox slots each sample consumed; a skipped sample is counted once in *skipped
hipError_t launch_cbowdev_draw(const DevGraph& g, const int32_t* field, uint64_t seed, uint64_t begin, uint64_t count,
                               int E, int N, int32_t* rec, uint8_t* clean, uint32_t* slots,
                               unsigned long long* skipped, hipStream_t st);

// ---------------------------------------------------------------- update kernels
// The kernels that turn records into row updates: edge_train_kernel and
// pair_train_kernel (edge_kernels.h), go_rec_kernel and go_pair_kernel
// (go_rec.h), warp_train_kernel (warp_kernels.h), hoprec_train_kernel
// (hoprec_kernels.h), skewopt_train_kernel (skewopt_kernels.h), cse_train_kernel
// (cse_kernels.h), cbow_train_kernel (cbow_kernels.h), eco_train_kernel
// (eco_kernels.h), cbowdev_train_kernel (cbowdev_kernels.h).  Each takes its argument
// struct as its one by-value parameter and exists per scatter MODE, KMAX
// bucket and (G, M) lane layout.

// (G, M) pairs for dpad in [4, 512]: G = min(64, pow2ceil(dpad / 4)) lanes,
// M = 4 * ceil(dpad / 4 / G) registers (lanes_of / regs_of; oracle
// orc_lane_width)
#define SMORE_FOR_EACH_GM(X) \
    X(1, 4) X(2, 4) X(4, 4) X(8, 4) X(16, 4) X(32, 4) X(64, 4) X(64, 8)

enum class KernelFamily { Edge, Pair, GoRec, GoPair, Warp, HopRec, SkewOpt, Cse, Cbow, Eco, CbowDev };

// Every (family, MODE, KMAX) instantiation.  Each is built in a unit of its
// own (train_edge_<mode>_k<KMAX>.hip, train_pair_<s|a|h><KMAX>.hip,
// train_warp_<s|a>.hip, train_hoprec_<s|a>.hip, train_skewopt_<s|a>.hip; train_go_rec_<s|a|h>.hip holds a
// mode's four Go ones, train_cse_<s|a>.hip a mode's nemf and nerank: KMAX = the direct negatives,
// train_cbow_<s|a>.hip: KMAX = the gather batch, train_eco_<s|a>.hip a mode's three K buckets,
// train_cbowdev_<s|a>.hip: KMAX = the bag's gather batch),
// so a new bucket is one line here and its .hip file.
#define SMORE_FOR_EACH_UPDATE_KERNEL(X)                                             \
    X(Edge, MODE_STORE, 5) X(Edge, MODE_STORE, 10) X(Edge, MODE_STORE, 20)          \
    X(Edge, MODE_ATOMIC, 5) X(Edge, MODE_ATOMIC, 10) X(Edge, MODE_ATOMIC, 20)       \
    X(Edge, MODE_HYBRID, 5) X(Edge, MODE_HYBRID, 10) X(Edge, MODE_HYBRID, 20)       \
    X(Pair, MODE_STORE, 5) X(Pair, MODE_STORE, 10)                                  \
    X(Pair, MODE_ATOMIC, 5) X(Pair, MODE_ATOMIC, 10)                                \
    X(Pair, MODE_HYBRID, 5) X(Pair, MODE_HYBRID, 10)                                \
    X(GoRec, MODE_STORE, 5) X(GoRec, MODE_STORE, 10)                                \
    X(GoRec, MODE_ATOMIC, 5) X(GoRec, MODE_ATOMIC, 10)                              \
    X(GoRec, MODE_HYBRID, 5) X(GoRec, MODE_HYBRID, 10)                              \
    X(GoPair, MODE_STORE, 5) X(GoPair, MODE_STORE, 10)                              \
    X(GoPair, MODE_ATOMIC, 5) X(GoPair, MODE_ATOMIC, 10)                            \
    X(GoPair, MODE_HYBRID, 5) X(GoPair, MODE_HYBRID, 10)                            \
    X(Warp, WARP_STORE, WARP_KMAX) X(Warp, WARP_ATOMIC, WARP_KMAX)                  \
    X(HopRec, MODE_STORE, HOPREC_KMAX) X(HopRec, MODE_ATOMIC, HOPREC_KMAX)          \
    X(SkewOpt, MODE_STORE, SKEWOPT_KMAX) X(SkewOpt, MODE_ATOMIC, SKEWOPT_KMAX)      \
    X(Cse, MODE_STORE, CSE_NEG) X(Cse, MODE_ATOMIC, CSE_NEG)                        \
    X(Cse, MODE_STORE, CSE_RANK_NEG) X(Cse, MODE_ATOMIC, CSE_RANK_NEG)              \
    X(Cbow, MODE_STORE, CBOW_BATCH) X(Cbow, MODE_ATOMIC, CBOW_BATCH)                \
    X(Eco, MODE_STORE, 5) X(Eco, MODE_STORE, 10) X(Eco, MODE_STORE, 20)             \
    X(Eco, MODE_ATOMIC, 5) X(Eco, MODE_ATOMIC, 10) X(Eco, MODE_ATOMIC, 20)          \
    X(CbowDev, MODE_STORE, CBOWDEV_BATCH) X(CbowDev, MODE_ATOMIC, CBOWDEV_BATCH)

// The instantiation's kernel for dpad's lane layout (Edge: and the model's
// rule), or nullptr when there is none: a (G, M) outside the list, BPR with
// KMAX != 5.  Specialised by the instantiation's unit (SMORE_UPDATE_INST).
template <KernelFamily F, int MODE, int KMAX>
const void* update_symbol(int dpad, int model);
#define X(F, MODE, KMAX) \
    template <>          \
    const void* update_symbol<KernelFamily::F, MODE, KMAX>(int dpad, int model);
SMORE_FOR_EACH_UPDATE_KERNEL(X)
#undef X
// in a unit: the specialisation, from the family's (G, M) ladder
// ladder<KMAX, MODE>(dpad, model) (edge_inst.h, go_rec.h, warp_kernels.h)
#define SMORE_UPDATE_INST(F, MODE, KMAX, ladder)                                          \
    namespace smore {                                                                     \
    template <>                                                                           \
    const void* update_symbol<KernelFamily::F, MODE, KMAX>(int dpad, int model) {         \
        return ladder<KMAX, MODE>(dpad, model);                                           \
    }                                                                                     \
    }

// What a driver with EdgeArgs asks for.  Cpp: pair records (alpha_rec 1) in a
// parallel mode with K <= 10 and !rec_edge go to pair_train_kernel, everything
// else, serial included, to edge_train_kernel.  (WARP resolves from its WarpArgs.)
enum class UpdateFamily { Cpp, GoRec, GoPair };

// a resolved kernel: fn == nullptr means no such instantiation (the launch
// fails with hipErrorInvalidValue); lds: the dynamic LDS of a hybrid launch
struct UpdateKernel {
    const void* fn;
    size_t lds;
};
UpdateKernel update_kernel(UpdateFamily f, const EdgeArgs& a);
UpdateKernel update_kernel(const WarpArgs& a);
UpdateKernel update_kernel(const HopRecArgs& a);
UpdateKernel update_kernel(const SkewOptArgs& a);
UpdateKernel update_kernel(const CseArgs& a);
UpdateKernel update_kernel(const CbowArgs& a);
UpdateKernel update_kernel(const EcoArgs& a);
UpdateKernel update_kernel(const CbowDevArgs& a);

// the one launch of the update kernels: 256 threads, `a` as the kernel's parameter
template <class Args>
hipError_t launch_update(const UpdateKernel& k, const Args& a, int grid, hipStream_t st) {
    if (!k.fn) return hipErrorInvalidValue;
    void* p[] = {(void*)&a};
    (void)hipLaunchKernel(k.fn, dim3(grid), dim3(256), p, k.lds, st);
    return hipGetLastError();
}

hipError_t launch_sample(const DevGraph& g, uint64_t seed, uint64_t begin, uint64_t count, int K,
                         int bpr, int32_t* out, hipStream_t st);
// 2-D block schedule (train_blocks.hip, blocks.cpp): C blocks <= BLOCK_MAX (N <= 16 W parts)
constexpr int BLOCK_MAX = 32;
struct BlockArgs {
    const uint4* atoms;       // LINE-2: this part's atoms, 2 uint4 each {thr, v, c, 0}, {v', c', 0, 0} (tagged ids)
    uint64_t atom_off;        // first atom of the launch's block
    uint32_t natoms;          // atoms of the launch's block
    const uint2* ntab;        // V entries: block k's negative alias over its vertices [cb[k], cb[k+1])
    int nb;                   // C blocks
    int32_t cb[BLOCK_MAX + 1];
    // hub C rows (blocks.cpp): slots V .. V + H - 1, drawn in every block.  A
    // block's negative alias runs over its rows then the H slots (entries
    // hub_ntab[k * H + j]); a LINE-2 sample takes a hub atom of the part
    // (atoms [hub_off, hub_off + nhub)) iff Philox word 2 < hub_thr.
    const uint2* hub_ntab;
    uint64_t hub_off;
    uint32_t nhub, hub_thr;
    int32_t H, V;
    // walk cells: per vertex -1, or its hub slot j | hot tag << 30; a pair
    // whose context is a hub goes to block (walk + center position) mod nb
    // (a center's hub pairs stay together) as slot id V + j
    const int32_t* hub_of;
};
hipError_t launch_block_draw(const BlockArgs& b, int blk, uint64_t seed, uint64_t begin, uint64_t count, int K,
                             int32_t* rec, hipStream_t st);
// rows idx[0 .. n) of T to out (gather) / from in (scatter), dpad floats each
hipError_t launch_rows_gather(const float* T, const int32_t* idx, uint64_t n, int dpad, float* out, hipStream_t st);
hipError_t launch_rows_scatter(float* T, const int32_t* idx, uint64_t n, int dpad, const float* in, hipStream_t st);
hipError_t launch_block_pair_count(const WalkArgs& w, const BlockArgs& b, uint64_t seed, uint32_t* count,
                                   hipStream_t st);
hipError_t launch_block_pair_emit(const WalkArgs& w, const BlockArgs& b, uint64_t seed, int K, double alpha0,
                                  const uint64_t* off, int32_t* rec, hipStream_t st);
// rows `ids` of T [*][dpad] from (to_table 1) / to (0) buf [n][dim] (membw.hip)
hipError_t launch_rows_io(float* T, const int32_t* ids, uint64_t n, int dpad, int dim, float* buf, int to_table,
                          hipStream_t st);
hipError_t launch_rows_put_sel(float* T, const int32_t* ids, const int32_t* pos, uint64_t m, int dpad, int dim,
                               const float* buf, hipStream_t st);
// streaming copy of n16 16-B words (membw.hip); variant 1 = non-temporal
hipError_t launch_copy(const void* src, void* dst, uint64_t n16, int blocks, int variant, hipStream_t st);
hipError_t launch_init_uniform(float* T, int64_t rows, int dim, int dpad, uint64_t seed,
                               hipStream_t st);

}  // namespace smore

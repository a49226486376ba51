/* cbow_spec.c -- the set-sum (CBOW) rule of GCN and TEXTGCN (GCN::Train,
 * src/model/GCN.cpp:62-117, TEXTGCN::Train, src/model/TEXTGCN.cpp:89-144, with
 * proNet::UpdateCBOW, src/proNet.cpp:2868-3001, and Opt_SigmoidRegSGD
 * :1332-1351) written once and instantiated twice: in the reference's fp64
 * arithmetic and in the project's fp32 arithmetic spec.  Test
 * infrastructure: compiled by tests/cbow_spec.py at run time and linked with
 * oracle/build/liboracle.so.
 *
 * One table W (w_vertex; w_context is never trained).  Sample s is unit s of
 * Philox stream 0, its slots consumed consecutively in the order of the
 * reference's random_gen calls: source attempts 2 slots each (p, index) until
 * field[v1] == 0; TEXTGCN (model 1) then v2 = TargetSample(v1), 2 slots (none
 * and -1 for a vertex without out-edge); GCN (model 0): vertex = context = v1,
 * TEXTGCN: vertex = v2, context = v1.  Then the c-set, S x TargetSample(context),
 * and the w-set, S x TargetSample(vertex) (every draw from the same vertex; a
 * vertex without out-edge gives an empty set and takes no slot); then K sets
 * of S uniform indices, one slot per attempt, each repeated until field == 1
 * (at most 2^16 attempts).  None of the draws looks at the table, so they are
 * made first (cbow_draw) and the rule runs on the record
 *   {vertex, context, c-set[S], w-set[S], K x neg-set[S]}
 * 2 + 2S + KS words, padded to a multiple of 4; an empty set is S times -1.
 * A sample without v2, with both sets empty, or with an exhausted rejection
 * loop is skipped: its record is all -1.
 *
 * The update works on the table in place in the reference's order: a set is
 * summed in set order from zero, the set's rows then take the same delta one
 * after the other (an id that occurs twice takes it twice), w_avg is computed
 * once, the w-set takes back_err last.
 *
 * The two instances differ only in the macros below:
 *   fp64: the reference's expressions as written
 *   fp32: alpha and reg rounded to fp32; a set sum is sequential fp32 adds from
 *         +0.0f; f = lane-order sum (G = orc_lane_width lanes, an fmaf chain
 *         per lane, then a pairwise tree); g = label - sig(f); a = alpha * g,
 *         r = alpha * reg; back_err = fmaf(-r, w_avg, fmaf(a, c_avg, back_err));
 *         back_c = fmaf(a, w_avg, -(r * c_avg)); row = row + delta.
 *   The sigmoid bucket of the fp32 f is found in fp64, its entry rounded to fp32.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "smore_oracle.h"

#define CBOW_MAX_S 10
#define CBOW_MAX_K 20
#define CBOW_ATTEMPTS (1u << 16)

static inline uint32_t draw_index(uint32_t k, uint64_t n) { return (uint32_t)(((uint64_t)k * n) >> 32); }

typedef struct {
    const orc_graph* g;
    uint64_t seed, unit;
    uint32_t slot;
} unit_words;
static uint32_t next_word(unit_words* u) { return orc_word(u->seed, 0, u->unit, u->slot++); }
/* SourceSample src/proNet.cpp:647-657 (p, then index) */
static int32_t source_sample(unit_words* u) {
    const orc_graph* g = u->g;
    uint32_t kp = next_word(u), ki = next_word(u);
    uint32_t i = draw_index(ki, (uint64_t)g->V);
    return kp < g->vthr[i] ? (int32_t)i : g->valias[i];
}
/* TargetSample src/proNet.cpp:671-683 (no out-edge: -1 before any draw; p, then index) */
static int32_t target_sample(unit_words* u, int32_t v) {
    const orc_graph* g = u->g;
    int64_t off = g->offsets[v], br = g->offsets[v + 1] - off;
    if (br == 0) return -1;
    uint32_t kp = next_word(u), ki = next_word(u);
    int64_t i = off + draw_index(ki, (uint64_t)br);
    return kp < g->cthr[i] ? g->targets[i] : g->calias[i];
}

int cbow_nwords(int S, int K) { return 2 + 2 * S + K * S; }
int cbow_width(int S, int K) { return (cbow_nwords(S, K) + 3) & ~3; }

/* the draws of sample s into rec (cbow_width words).  Returns 0: a sample, 1:
 * skipped (rec all -1).  *slots: the slots consumed. */
int cbow_draw(const orc_graph* g, const int32_t* field, uint64_t seed, uint64_t s, int model, int S, int K,
              int32_t* rec, uint32_t* slots) {
    const int RW = cbow_width(S, K);
    unit_words u = {g, seed, s, 0};
    int skip = 0;
    for (int k = 0; k < RW; ++k) rec[k] = -1;
    int32_t v1 = -1, vertex, context;
    uint32_t a;
    for (a = 0; a < CBOW_ATTEMPTS; ++a) {
        v1 = source_sample(&u);
        if (field[v1] == 0) break;
    }
    if (a == CBOW_ATTEMPTS) skip = 1;
    if (!skip) {
        context = v1;
        vertex = model ? target_sample(&u, v1) : v1;
        if (vertex < 0) skip = 1;
    }
    if (!skip) {
        rec[0] = vertex;
        rec[1] = context;
        for (int p = 0; p < 2; ++p) {
            int32_t* o = rec + 2 + p * S;
            for (int i = 0; i < S; ++i) {
                o[i] = target_sample(&u, p ? vertex : context);
                if (o[i] < 0) break;   /* the first draw: the vertex has no out-edge */
            }
        }
        if (rec[2] < 0 && rec[2 + S] < 0) skip = 1;
    }
    for (int n = 0; !skip && n < K * S; ++n) {
        int32_t j = -1;
        for (a = 0; a < CBOW_ATTEMPTS; ++a) {
            j = (int32_t)draw_index(next_word(&u), (uint64_t)g->V);
            if (field[j] == 1) break;
        }
        if (a == CBOW_ATTEMPTS) skip = 1;
        rec[2 + 2 * S + n] = j;
    }
    if (skip)
        for (int k = 0; k < RW; ++k) rec[k] = -1;
    if (slots) *slots = u.slot;
    return skip;
}

/* clean: the c-set ids and all K S negative ids are pairwise distinct */
int cbow_clean(const int32_t* rec, int S, int K) {
    int32_t id[CBOW_MAX_S * (CBOW_MAX_K + 1)];
    int n = 0;
    for (int i = 0; i < S; ++i)
        if (rec[2 + i] >= 0) id[n++] = rec[2 + i];
    for (int i = 0; i < K * S; ++i) id[n++] = rec[2 + 2 * S + i];
    for (int i = 1; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (id[i] == id[j]) return 0;
    return 1;
}

static double dot_f64(const double* a, const double* b, int d) {
    double f = 0.0;
    for (int k = 0; k < d; ++k) f += a[k] * b[k];
    return f;
}

static float dot_f32(const float* a, const float* b, int dpad) {
    float part[64];
    int G = orc_lane_width(dpad);
    for (int l = 0; l < G; ++l) {
        float p = 0.0f;
        for (int q = l; q < dpad / 4; q += G)
            for (int e = 4 * q; e < 4 * q + 4; ++e) p = fmaf(a[e], b[e], p);
        part[l] = p;
    }
    for (int w = 1; w < G; w <<= 1)
        for (int l = 0; l < G; l += 2 * w) part[l] = part[l] + part[l + w];
    return part[0];
}

/* fastSigmoid's table index (src/proNet.cpp:62-71): -1 below -8, 1001 above 8 */
static int bucket_of(double x) {
    if (x < -8.0) return -1;
    if (x > 8.0) return 1001;
    return (int)((x + 8.0) * 1000 / 8.0 / 2);
}

/* the rule.  W: V rows of `d` REALs (fp32: d = dpad, padding zero); W == NULL:
 * the draws only.  Samples [begin, end).  Per sample (each array may be NULL):
 * rec cbow_width words; slots: slots the draws consumed; used: slots the
 * reference consumes (the same: every draw is made whatever the table holds);
 * bucket: 1 + K sigmoid buckets (positive step, then the negative steps; -2 for
 * a skipped sample); clean: 1 clean, 0 ordered, -1 skipped.  Returns the
 * samples skipped. */
#define CBOW_SPEC(NAME, REAL, DOT, UPD)                                                                            \
    int NAME(const orc_graph* g, const int32_t* field, REAL* W, int d, int model, int S, int K, double alpha0,     \
             double reg0, uint64_t total, uint64_t begin, uint64_t end, uint64_t seed, int32_t* rec,               \
             uint32_t* slots, uint32_t* used, int32_t* bucket, int32_t* clean) {                                   \
        const int RW = cbow_width(S, K);                                                                           \
        REAL* w_avg = (REAL*)malloc(sizeof(REAL) * (size_t)(d > 0 ? d : 1) * 4);                                   \
        REAL *c_avg = w_avg + d, *back = w_avg + 2 * d, *back_c = w_avg + 3 * d;                                   \
        int32_t own[(2 + 2 * CBOW_MAX_S + CBOW_MAX_S * CBOW_MAX_K + 3) & ~3];                                      \
        int skipped = 0;                                                                                           \
        const REAL reg = (REAL)reg0;                                                                               \
        for (uint64_t s = begin; s < end; ++s) {                                                                   \
            int32_t* r = rec ? rec + (s - begin) * (uint64_t)RW : own;                                             \
            uint32_t sl;                                                                                           \
            const int sk = cbow_draw(g, field, seed, s, model, S, K, r, &sl);                                      \
            if (slots) slots[s - begin] = sl;                                                                      \
            if (used) used[s - begin] = sl;                                                                        \
            if (clean) clean[s - begin] = sk ? -1 : cbow_clean(r, S, K);                                           \
            if (bucket)                                                                                            \
                for (int k = 0; k <= K; ++k) bucket[(s - begin) * (uint64_t)(K + 1) + k] = -2;                     \
            if (sk) skipped++;                                                                                     \
            if (sk || !W) continue;                                                                                \
            const REAL alpha = (REAL)orc_alpha_line(s, alpha0, total);                                             \
            const int32_t* ws = r + 2 + S;                                                                         \
            for (int k = 0; k < d; ++k) w_avg[k] = back[k] = (REAL)0.0;                                            \
            for (int i = 0; i < S && ws[i] >= 0; ++i)                                                              \
                for (int k = 0; k < d; ++k) w_avg[k] = w_avg[k] + W[(int64_t)ws[i] * d + k];                       \
            for (int st = 0; st <= K; ++st) {                                                                      \
                const int32_t* cs = st ? r + 2 + 2 * S + (st - 1) * S : r + 2;                                     \
                for (int k = 0; k < d; ++k) c_avg[k] = (REAL)0.0;                                                  \
                for (int i = 0; i < S && cs[i] >= 0; ++i)                                                          \
                    for (int k = 0; k < d; ++k) c_avg[k] = c_avg[k] + W[(int64_t)cs[i] * d + k];                   \
                const REAL f = DOT(w_avg, c_avg, d);                                                               \
                if (bucket) bucket[(s - begin) * (uint64_t)(K + 1) + st] = bucket_of((double)f);                   \
                const REAL gl = (st ? (REAL)0.0 : (REAL)1.0) - (REAL)orc_fast_sigmoid((double)f);                  \
                UPD(alpha, reg, gl, w_avg, c_avg, back, back_c, d)                                                 \
                for (int i = 0; i < S && cs[i] >= 0; ++i)                                                          \
                    for (int k = 0; k < d; ++k) W[(int64_t)cs[i] * d + k] = W[(int64_t)cs[i] * d + k] + back_c[k]; \
            }                                                                                                      \
            for (int i = 0; i < S && ws[i] >= 0; ++i)                                                              \
                for (int k = 0; k < d; ++k) W[(int64_t)ws[i] * d + k] = W[(int64_t)ws[i] * d + k] + back[k];       \
        }                                                                                                          \
        free(w_avg);                                                                                               \
        return skipped;                                                                                            \
    }

/* fp64: Opt_SigmoidRegSGD as written; back_c_err is zero when it is called, and that sum is kept */
#define UPD64(al, reg, gl, w, c, back, bc, d)                                                \
    for (int k = 0; k < d; ++k) back[k] += (al) * ((gl) * c[k] - (reg) * w[k]);              \
    for (int k = 0; k < d; ++k) bc[k] = 0.0 + (al) * ((gl) * w[k] - (reg) * c[k]);
#define UPD32(al, reg, gl, w, c, back, bc, d)                                                \
    {                                                                                        \
        const float a_ = (al) * (gl), r_ = (al) * (reg);                                     \
        for (int k = 0; k < d; ++k) back[k] = fmaf(-r_, w[k], fmaf(a_, c[k], back[k]));      \
        for (int k = 0; k < d; ++k) bc[k] = fmaf(a_, w[k], -(r_ * c[k]));                    \
    }

CBOW_SPEC(cbow_spec_f64, double, dot_f64, UPD64)
CBOW_SPEC(cbow_spec_f32, float, dot_f32, UPD32)

/* the rule's objective on one record: -log sigma(w_avg . c_avg) on the positive
 * sets, -log(1 - sigma) on each negative set (the exact sigmoid), summed over
 * the record's 1 + K terms; fp64 on a float64 table.  A skipped record gives 0. */
double cbow_loss(const double* W, int d, int S, int K, const int32_t* r) {
    if (r[0] < 0) return 0.0;
    double* w_avg = (double*)calloc((size_t)d * 2, sizeof(double));
    double* c_avg = w_avg + d;
    double loss = 0.0;
    const int32_t* ws = r + 2 + S;
    for (int i = 0; i < S && ws[i] >= 0; ++i)
        for (int k = 0; k < d; ++k) w_avg[k] += W[(int64_t)ws[i] * d + k];
    for (int st = 0; st <= K; ++st) {
        const int32_t* cs = st ? r + 2 + 2 * S + (st - 1) * S : r + 2;
        for (int k = 0; k < d; ++k) c_avg[k] = 0.0;
        for (int i = 0; i < S && cs[i] >= 0; ++i)
            for (int k = 0; k < d; ++k) c_avg[k] += W[(int64_t)cs[i] * d + k];
        const double f = dot_f64(w_avg, c_avg, d);
        /* -log sigma(x) = log1p(exp(-x)); -log(1 - sigma(x)) = log1p(exp(x)) */
        loss += log1p(exp(st ? f : -f));
    }
    free(w_avg);
    return loss;
}

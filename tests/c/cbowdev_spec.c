/* cbowdev_spec.c -- the bag-of-words event rule of TEXTGCNdev (TEXTGCNdev::Train,
 * src/model/TEXTGCNdev.cpp:71-126, with proNet::UpdateCBOWdev,
 * src/proNet.cpp:2755-2865, and Opt_SigmoidRegSGD :1332-1351) written once and
 * instantiated twice: in the reference's fp64 arithmetic and in the project's
 * fp32 arithmetic spec.  Test infrastructure: compiled by
 * tests/cbowdev_spec.py at run time and linked with oracle/build/liboracle.so.
 *
 * Two tables: W (w_vertex: user, event and negative rows, moved one at a time)
 * and C (w_context: the bag's rows, summed and given one shared delta).  Sample
 * s is unit s of Philox stream 0, its slots consumed consecutively in the order
 * of the reference's random_gen calls: source attempts 2 slots each (p, index)
 * until field[user] == 0; then E times event = TargetSample(user) followed by N
 * times word = TargetSample(event), 2 slots each (none, and -1, for a vertex
 * without out-edge: the sample ends there); then 10 E uniform indices, one slot
 * per attempt, each repeated until field == 1 (at most 2^16 attempts).  None of
 * the draws looks at a table, so they are made first (cbowdev_draw) and the rule
 * runs on the record
 *   {user, event, bag[E N], E x {a0, b0, .. a4, b4}}
 * 2 + E N + 10 E words, padded to a multiple of 4.  `event` is the LAST event
 * drawn: the reference's update loop uses the variable the collection loop
 * left behind.  A sample whose collection meets a -1, or with an exhausted
 * rejection loop, is skipped: its record is all -1.
 *
 * The rule keeps the reference's accidents: label is 1 in
 * iteration 0 only, five negative pairs per iteration whatever the flags say,
 * and a step updates its row in place before the second loop of the same step
 * reads it.
 *
 * The two instances differ only in the macros below:
 *   fp64: the reference's expressions as written
 *   fp32: alpha and reg rounded to fp32; w_avg is sequential fp32 adds from
 *         +0.0f in bag order; f = lane-order sum (G = orc_lane_width lanes, an
 *         fmaf chain per lane, then a pairwise tree); g = label - sig(f);
 *         a = alpha * g, r = alpha * reg; d = fmaf(a, ctx, -(r * row));
 *         row' = row + d; acc = fmaf(-r, ctx, fmaf(a, row', acc)); the closing
 *         writes are row + delta.
 *   The sigmoid bucket of the fp32 f is found in fp64, its entry rounded to fp32.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "smore_oracle.h"

#define CBOWDEV_MAX 10
#define CBOWDEV_NEG 5
#define CBOWDEV_ATTEMPTS (1u << 16)

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

int cbowdev_nwords(int E, int N) { return 2 + E * N + 2 * CBOWDEV_NEG * E; }
int cbowdev_width(int E, int N) { return (cbowdev_nwords(E, N) + 3) & ~3; }

/* the draws of sample s into rec (cbowdev_width words).  Returns 0: a sample, 1:
 * skipped (rec all -1).  *slots: the slots consumed.  events (or NULL): the E
 * events of the collection loop, -1 from the one that was not drawn. */
int cbowdev_draw(const orc_graph* g, const int32_t* field, uint64_t seed, uint64_t s, int E, int N, int32_t* rec,
                 uint32_t* slots, int32_t* events) {
    const int RW = cbowdev_width(E, N);
    unit_words u = {g, seed, s, 0};
    int skip = 0;
    for (int k = 0; k < RW; ++k) rec[k] = -1;
    if (events)
        for (int i = 0; i < E; ++i) events[i] = -1;
    int32_t user = -1, event = -1;
    uint32_t a;
    for (a = 0; a < CBOWDEV_ATTEMPTS; ++a) {
        user = source_sample(&u);
        if (field[user] == 0) break;
    }
    if (a == CBOWDEV_ATTEMPTS) skip = 1;
    for (int i = 0; !skip && i < E; ++i) {
        event = target_sample(&u, user);
        if (events) events[i] = event;
        if (event < 0) skip = 1;
        for (int j = 0; !skip && j < N; ++j) {
            const int32_t word = target_sample(&u, event);
            if (word < 0) skip = 1;
            rec[2 + i * N + j] = word;
        }
    }
    for (int n = 0; !skip && n < 2 * CBOWDEV_NEG * E; ++n) {
        int32_t j = -1;
        for (a = 0; a < CBOWDEV_ATTEMPTS; ++a) {
            j = (int32_t)draw_index(next_word(&u), (uint64_t)g->V);
            if (field[j] == 1) break;
        }
        if (a == CBOWDEV_ATTEMPTS) skip = 1;
        rec[2 + E * N + n] = j;
    }
    rec[0] = user;
    rec[1] = event;
    if (skip)
        for (int k = 0; k < RW; ++k) rec[k] = -1;
    if (slots) *slots = u.slot;
    return skip;
}

/* clean: user, event and the 10 E negative ids are pairwise distinct (the bag ids
 * address the other table) */
int cbowdev_clean(const int32_t* rec, int E, int N) {
    int32_t id[2 + 2 * CBOWDEV_NEG * CBOWDEV_MAX];
    int n = 0;
    id[n++] = rec[0];
    id[n++] = rec[1];
    for (int i = 0; i < 2 * CBOWDEV_NEG * E; ++i) id[n++] = rec[2 + E * N + i];
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

/* Opt_SigmoidRegSGD(row, ctx, label, alpha, reg, row, acc): the row is its own loss vector, so
 * it is updated in place and the second loop reads it as updated (ctx too, where ctx == row) */
#define STEP64(al, reg, gl, row, ctx, acc, d)                                                \
    for (int k = 0; k < d; ++k) row[k] += (al) * ((gl) * ctx[k] - (reg) * row[k]);           \
    for (int k = 0; k < d; ++k) acc[k] += (al) * ((gl) * row[k] - (reg) * ctx[k]);
#define STEP32(al, reg, gl, row, ctx, acc, d)                                                \
    {                                                                                        \
        const float a_ = (al) * (gl), r_ = (al) * (reg);                                     \
        for (int k = 0; k < d; ++k) row[k] = row[k] + fmaf(a_, ctx[k], -(r_ * row[k]));      \
        for (int k = 0; k < d; ++k) acc[k] = fmaf(-r_, ctx[k], fmaf(a_, row[k], acc[k]));    \
    }

/* the rule.  W, C: V rows of `d` REALs each (fp32: d = dpad, padding zero); W == NULL: the draws
 * only.  Samples [begin, end).  Per sample (each array may be NULL): rec cbowdev_width words;
 * slots: slots the draws consumed; used: slots the reference consumes (the same); bucket: the
 * 12 E sigmoid buckets in step order (-2 for a skipped sample); clean: 1 clean, 0 ordered, -1
 * skipped.  Returns the samples skipped. */
#define CBOWDEV_SPEC(NAME, REAL, DOT, STEP)                                                                        \
    int NAME(const orc_graph* g, const int32_t* field, REAL* W, REAL* C, int d, int E, int N, double alpha0,      \
             double reg0, uint64_t total, uint64_t begin, uint64_t end, uint64_t seed, int32_t* rec,              \
             uint32_t* slots, uint32_t* used, int32_t* bucket, int32_t* clean) {                                  \
        const int RW = cbowdev_width(E, N), NS = 12 * E;                                                          \
        REAL* w_avg = (REAL*)malloc(sizeof(REAL) * (size_t)(d > 0 ? d : 1) * 3);                                  \
        REAL *back = w_avg + d, *uerr = w_avg + 2 * d;                                                            \
        int32_t own[(2 + CBOWDEV_MAX * CBOWDEV_MAX + 2 * CBOWDEV_NEG * CBOWDEV_MAX + 3) & ~3];                    \
        int skipped = 0;                                                                                          \
        const REAL reg = (REAL)reg0;                                                                              \
        for (uint64_t s = begin; s < end; ++s) {                                                                  \
            int32_t* r = rec ? rec + (s - begin) * (uint64_t)RW : own;                                            \
            uint32_t sl;                                                                                          \
            const int sk = cbowdev_draw(g, field, seed, s, E, N, r, &sl, NULL);                                   \
            if (slots) slots[s - begin] = sl;                                                                     \
            if (used) used[s - begin] = sl;                                                                       \
            if (clean) clean[s - begin] = sk ? -1 : cbowdev_clean(r, E, N);                                       \
            int32_t* bk = bucket ? bucket + (s - begin) * (uint64_t)NS : NULL;                                    \
            if (bk)                                                                                               \
                for (int k = 0; k < NS; ++k) bk[k] = -2;                                                          \
            if (sk) skipped++;                                                                                    \
            if (sk || !W) continue;                                                                               \
            const REAL alpha = (REAL)orc_alpha_line(s, alpha0, total);                                            \
            const int32_t *bag = r + 2, *neg = r + 2 + E * N;                                                     \
            REAL *wu = W + (int64_t)r[0] * d, *we = W + (int64_t)r[1] * d;                                        \
            for (int k = 0; k < d; ++k) w_avg[k] = back[k] = uerr[k] = (REAL)0.0;                                 \
            for (int i = 0; i < E * N; ++i)                                                                       \
                for (int k = 0; k < d; ++k) w_avg[k] = w_avg[k] + C[(int64_t)bag[i] * d + k];                     \
            REAL label = (REAL)1.0;                                                                               \
            int st = 0;                                                                                           \
            for (int i = 0; i < E; ++i) {                                                                         \
                for (int q = 0; q < 2 + 2 * CBOWDEV_NEG; ++q) {                                                   \
                    REAL* row = q < 2 ? we : W + (int64_t)neg[i * 2 * CBOWDEV_NEG + q - 2] * d;                   \
                    const REAL* ctx = (q & 1) ? wu : w_avg;                                                       \
                    REAL* acc = (q & 1) ? uerr : back;                                                            \
                    if (q == 2) label = (REAL)0.0;                                                                \
                    const REAL f = DOT(row, ctx, d);                                                              \
                    if (bk) bk[st] = bucket_of((double)f);                                                        \
                    st++;                                                                                         \
                    const REAL gl = label - (REAL)orc_fast_sigmoid((double)f);                                    \
                    STEP(alpha, reg, gl, row, ctx, acc, d)                                                        \
                }                                                                                                 \
            }                                                                                                     \
            for (int k = 0; k < d; ++k) wu[k] = wu[k] + uerr[k];                                                  \
            for (int i = 0; i < E * N; ++i)                                                                       \
                for (int k = 0; k < d; ++k) C[(int64_t)bag[i] * d + k] = C[(int64_t)bag[i] * d + k] + back[k];    \
        }                                                                                                         \
        free(w_avg);                                                                                              \
        return skipped;                                                                                           \
    }

CBOWDEV_SPEC(cbowdev_spec_f64, double, dot_f64, STEP64)
CBOWDEV_SPEC(cbowdev_spec_f32, float, dot_f32, STEP32)

/* the rule's objective on one record, the event term once and every negative pair (the exact
 * sigmoid): -log s(W[e].w_avg) - log s(W[e].W[u]) - sum log(1 - s(W[a].w_avg)) - sum log(1 -
 * s(W[b].W[u])); fp64 on float64 tables.  A skipped record gives 0. */
double cbowdev_loss(const double* W, const double* C, int d, int E, int N, const int32_t* r) {
    if (r[0] < 0) return 0.0;
    double* w_avg = (double*)calloc((size_t)d, sizeof(double));
    const double *wu = W + (int64_t)r[0] * d, *we = W + (int64_t)r[1] * d;
    for (int i = 0; i < E * N; ++i)
        for (int k = 0; k < d; ++k) w_avg[k] += C[(int64_t)r[2 + i] * d + k];
    /* -log sigma(x) = log1p(exp(-x)); -log(1 - sigma(x)) = log1p(exp(x)) */
    double loss = log1p(exp(-dot_f64(we, w_avg, d))) + log1p(exp(-dot_f64(we, wu, d)));
    for (int n = 0; n < 2 * CBOWDEV_NEG * E; ++n) {
        const double* row = W + (int64_t)r[2 + E * N + n] * d;
        loss += log1p(exp(dot_f64(row, (n & 1) ? wu : w_avg, d)));
    }
    free(w_avg);
    return loss;
}

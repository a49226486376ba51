/* eco_spec.c -- the sampled-softmax choice rule of ECO (ECO::Train,
 * src/model/ECO.cpp:64-128, with proNet::UpdateDChoice, src/proNet.cpp:2221-2341)
 * written twice: in the reference's fp64 arithmetic and in the project's fp32
 * arithmetic spec.  Test infrastructure: compiled by
 * tests/eco_spec.py at run time and linked with oracle/build/liboracle.so.
 *
 * One table W (w_vertex; w_ignore is never touched).  Sample s is unit s of
 * Philox stream 0, its slots consumed consecutively in the order of the
 * reference's random_gen calls: source attempts 2 slots each (p, index) until
 * field[v] == 0; v2 = TargetSample(v), 2 slots, thrown away; then five lists of
 * c1 = TargetSample(v), x = TargetSample(c1), c2 = TargetSample(x) (2 slots
 * each) and K NegativeSamples (2 slots each: index, p).  None of the draws
 * looks at the table, so they are made first (eco_draw) and the rule runs on
 * the record {v, 5 x {c1, c2, n_0..n_{K-1}}}, 1 + 5 (2 + K) words padded to a
 * multiple of 4.  A sample one of whose TargetSamples returns -1 (the draws
 * stop there) or whose source loop gave up after 2^16 attempts is skipped: its
 * record is all -1.
 *
 * The update works on the table in place and reads a row from the table every
 * time the reference does, so ids that coincide see the earlier writes.
 *   fp64: the reference's expressions as written, libm exp.
 *   fp32: alpha and reg rounded to fp32; a score is the lane-order dot (G =
 *         orc_lane_width lanes, an fmaf chain per lane, a pairwise tree) through
 *         exp32 (smore_amd/csrc/exp32.h); sum = ((0 + e_0) + ..) + e1 + e2;
 *         dev = fmaf(W[n_k], e_k, .. fmaf(W[c2], e2, W[c1] e1)); is = 1 / sum,
 *         id = 1 / ((e1 + e1) + e2) (IEEE divisions), g1 = (e1 + e1) id, g2 = e2 id;
 *         back_v = fmaf(alpha, fmaf(-reg, W[v], fmaf(-is, dev, fmaf(g1, W[c1], g2 W[c2]))), back_v);
 *         a row x with coefficient cf (c1: g1 - e1 is, c2: g2 - e2 is, n_k: -(e_k is)) becomes
 *         W[x] + alpha fmaf(-reg, W[x], cf W[v]); W[v] = W[v] + back_v.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "exp32.h"
#include "smore_oracle.h"

#define ECO_LISTS 5
#define ECO_MAX_K 20
#define ECO_ATTEMPTS (1u << 16)

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
/* NegativeSample src/proNet.cpp:623-633 (index, then p) */
static int32_t negative_sample(unit_words* u) {
    const orc_graph* g = u->g;
    uint32_t ki = next_word(u), kp = next_word(u);
    uint32_t i = draw_index(ki, (uint64_t)g->V);
    return kp < g->nthr[i] ? (int32_t)i : g->nalias[i];
}

int eco_nwords(int K) { return 1 + ECO_LISTS * (2 + K); }
int eco_width(int K) { return (eco_nwords(K) + 3) & ~3; }

/* the draws of sample s into rec (eco_width words).  Returns 0: a sample, 1:
 * skipped (rec all -1).  *slots: the slots consumed. */
int eco_draw(const orc_graph* g, const int32_t* field, uint64_t seed, uint64_t s, int K, int32_t* rec, uint32_t* slots) {
    const int RW = eco_width(K);
    unit_words u = {g, seed, s, 0};
    int skip = 0;
    for (int k = 0; k < RW; ++k) rec[k] = -1;
    int32_t v = -1;
    uint32_t a;
    for (a = 0; a < ECO_ATTEMPTS; ++a) {
        v = source_sample(&u);
        if (field[v] == 0) break;
    }
    if (a == ECO_ATTEMPTS) skip = 1;
    if (!skip && target_sample(&u, v) < 0) skip = 1;
    if (!skip) rec[0] = v;
    for (int l = 0; !skip && l < ECO_LISTS; ++l) {
        int32_t* o = rec + 1 + l * (2 + K);
        int32_t c1 = target_sample(&u, v);
        int32_t c2 = c1 < 0 ? -1 : target_sample(&u, c1);
        if (c2 >= 0) c2 = target_sample(&u, c2);
        if (c2 < 0) {
            skip = 1;
            break;
        }
        o[0] = c1;
        o[1] = c2;
        for (int k = 0; k < K; ++k) o[2 + k] = negative_sample(&u);
    }
    if (skip)
        for (int k = 0; k < RW; ++k) rec[k] = -1;
    if (slots) *slots = u.slot;
    return skip;
}

/* clean: all 1 + 5 (2 + K) ids are pairwise distinct */
int eco_clean(const int32_t* rec, int K) {
    const int n = eco_nwords(K);
    for (int i = 1; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (rec[i] == rec[j]) return 0;
    return 1;
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

/* UpdateDChoice on record r, the reference's expressions */
static void update_f64(double* W, int d, const int32_t* r, int K, double alpha, double reg, double* back_v) {
    const int64_t vertex = r[0];
    double neg_scores[ECO_MAX_K];
    for (int k = 0; k < d; ++k) back_v[k] = 0.0;
    for (int b = 0; b < ECO_LISTS; ++b) {
        const int32_t* set = r + 1 + b * (2 + K);
        const int64_t context = set[0], context2 = set[1];
        double pos_score = 0.0, pos_score2 = 0.0, sum_score = 0.0;
        for (int k = 0; k < d; ++k) {
            pos_score += W[vertex * d + k] * W[context * d + k];
            pos_score2 += W[vertex * d + k] * W[context2 * d + k];
        }
        for (int n = 0; n < K; ++n) {
            const int64_t neg_item = set[2 + n];
            double neg_score = 0.0;
            for (int k = 0; k < d; ++k) neg_score += W[vertex * d + k] * W[neg_item * d + k];
            neg_score = exp(neg_score);
            neg_scores[n] = neg_score;
            sum_score += neg_score;
        }
        pos_score = exp(pos_score);
        pos_score2 = exp(pos_score2);
        sum_score += pos_score;
        sum_score += pos_score2;
        for (int k = 0; k < d; ++k) {
            const double dev_p1 = W[context * d + k] * pos_score;
            const double dev_p2 = W[context2 * d + k] * pos_score2;
            double dev = dev_p1 + dev_p2;
            for (int n = 0; n < K; ++n) dev += W[(int64_t)set[2 + n] * d + k] * neg_scores[n];
            back_v[k] += alpha * ((2.0 * dev_p1 + dev_p2) / (2.0 * pos_score + pos_score2) - dev / sum_score -
                                  reg * W[vertex * d + k]);
        }
        for (int k = 0; k < d; ++k) {
            W[context * d + k] += alpha * ((2.0 * W[vertex * d + k] * pos_score) / (2.0 * pos_score + pos_score2) -
                                           (W[vertex * d + k] * pos_score) / sum_score - reg * W[context * d + k]);
            W[context2 * d + k] += alpha * ((W[vertex * d + k] * pos_score2) / (2.0 * pos_score + pos_score2) -
                                            (W[vertex * d + k] * pos_score2) / sum_score - reg * W[context2 * d + k]);
        }
        for (int n = 0; n < K; ++n) {
            const int64_t neg_item = set[2 + n];
            for (int k = 0; k < d; ++k)
                W[neg_item * d + k] -= alpha * ((W[vertex * d + k] * neg_scores[n]) / sum_score + reg * W[neg_item * d + k]);
        }
    }
    for (int k = 0; k < d; ++k) W[vertex * d + k] += back_v[k];
}

/* the same in the fp32 arithmetic spec; d = dpad, padding zero */
static void move_f32(float* W, int d, int64_t x, int64_t v, float cf, float alpha, float reg) {
    for (int k = 0; k < d; ++k) W[x * d + k] = W[x * d + k] + alpha * fmaf(-reg, W[x * d + k], cf * W[v * d + k]);
}
static void update_f32(float* W, int d, const int32_t* r, int K, float alpha, float reg, float* back_v) {
    const int64_t v = r[0];
    float e[ECO_MAX_K];
    float* dev = back_v + d;
    for (int k = 0; k < d; ++k) back_v[k] = 0.0f;
    for (int b = 0; b < ECO_LISTS; ++b) {
        const int32_t* set = r + 1 + b * (2 + K);
        const int64_t c1 = set[0], c2 = set[1];
        const float e1 = exp32(dot_f32(W + v * d, W + c1 * d, d)), e2 = exp32(dot_f32(W + v * d, W + c2 * d, d));
        float sum = 0.0f;
        for (int k = 0; k < d; ++k) dev[k] = fmaf(W[c2 * d + k], e2, W[c1 * d + k] * e1);
        for (int n = 0; n < K; ++n) {
            const int64_t x = set[2 + n];
            e[n] = exp32(dot_f32(W + v * d, W + x * d, d));
            sum = sum + e[n];
            for (int k = 0; k < d; ++k) dev[k] = fmaf(W[x * d + k], e[n], dev[k]);
        }
        sum = sum + e1;
        sum = sum + e2;
        const float is = 1.0f / sum, e11 = e1 + e1, id = 1.0f / (e11 + e2);
        const float g1 = e11 * id, g2 = e2 * id;
        const float cf1 = g1 - e1 * is, cf2 = g2 - e2 * is;
        for (int k = 0; k < d; ++k) {
            const float t = fmaf(-is, dev[k], fmaf(g1, W[c1 * d + k], g2 * W[c2 * d + k]));
            back_v[k] = fmaf(alpha, fmaf(-reg, W[v * d + k], t), back_v[k]);
        }
        move_f32(W, d, c1, v, cf1, alpha, reg);
        move_f32(W, d, c2, v, cf2, alpha, reg);
        for (int n = 0; n < K; ++n) move_f32(W, d, set[2 + n], v, -(e[n] * is), alpha, reg);
    }
    for (int k = 0; k < d; ++k) W[v * d + k] = W[v * d + k] + back_v[k];
}

/* the rule.  W: V rows of `d` REALs (fp32: d = dpad, padding zero); W == NULL:
 * the draws only.  Samples [begin, end).  Per sample (each array may be NULL):
 * rec eco_width words; slots: slots the draws consumed; clean: 1 clean, 0
 * ordered, -1 skipped.  Returns the samples skipped. */
#define ECO_SPEC(NAME, REAL, UPDATE)                                                                              \
    int NAME(const orc_graph* g, const int32_t* field, REAL* W, int d, int K, double alpha0, double reg0,         \
             uint64_t total, uint64_t begin, uint64_t end, uint64_t seed, int32_t* rec, uint32_t* slots,          \
             int32_t* clean) {                                                                                    \
        const int RW = eco_width(K);                                                                              \
        REAL* tmp = (REAL*)malloc(sizeof(REAL) * (size_t)(d > 0 ? d : 1) * 2);                                    \
        int32_t own[(1 + ECO_LISTS * (2 + ECO_MAX_K) + 3) & ~3];                                                  \
        int skipped = 0;                                                                                          \
        for (uint64_t s = begin; s < end; ++s) {                                                                  \
            int32_t* r = rec ? rec + (s - begin) * (uint64_t)RW : own;                                            \
            uint32_t sl;                                                                                          \
            const int sk = eco_draw(g, field, seed, s, K, r, &sl);                                                \
            if (slots) slots[s - begin] = sl;                                                                     \
            if (clean) clean[s - begin] = sk ? -1 : eco_clean(r, K);                                              \
            if (sk) skipped++;                                                                                    \
            if (sk || !W) continue;                                                                               \
            UPDATE(W, d, r, K, (REAL)orc_alpha_line(s, alpha0, total), (REAL)reg0, tmp);                          \
        }                                                                                                         \
        free(tmp);                                                                                                \
        return skipped;                                                                                           \
    }

ECO_SPEC(eco_spec_f64, double, update_f64)
ECO_SPEC(eco_spec_f32, float, update_f32)

/* the rule's objective on one record: log(sum) - log(2 e1 + e2) summed over
 * the record's five lists; fp64 on a float64 table.  A skipped record gives 0. */
double eco_loss(const double* W, int d, int K, const int32_t* r) {
    if (r[0] < 0) return 0.0;
    const int64_t v = r[0];
    double loss = 0.0;
    for (int b = 0; b < ECO_LISTS; ++b) {
        const int32_t* set = r + 1 + b * (2 + K);
        double sc[2 + ECO_MAX_K], sum = 0.0;
        for (int j = 0; j < 2 + K; ++j) {
            double f = 0.0;
            for (int k = 0; k < d; ++k) f += W[v * d + k] * W[(int64_t)set[j] * d + k];
            sc[j] = exp(f);
            sum += sc[j];
        }
        loss += log(sum) - log(2.0 * sc[0] + sc[1]);
    }
    return loss;
}

/* exp32 over n evenly spaced arguments of [lo, hi] (fp32 values of lo + i (hi - lo) / (n - 1)):
 * the worst relative error against double exp; *at: where */
double eco_exp32_worst(double lo, double hi, int64_t n, double* at) {
    double worst = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        const float x = (float)(lo + (hi - lo) * (double)i / (double)(n - 1));
        const double want = exp((double)x), err = fabs((double)exp32(x) - want) / want;
        if (err > worst) {
            worst = err;
            if (at) *at = (double)x;
        }
    }
    return worst;
}
float eco_exp32(float x) { return exp32(x); }

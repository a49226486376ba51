/* skewopt_spec.c -- the Skew-OPT rule (SPR::Train, src/model/SkewOPT.cpp:88-93,
 * with proNet::UpdateSBPRPair, src/proNet.cpp:1517-1566, and Opt_SBPRSGD,
 * :1070-1098) written once and instantiated twice: in the reference's fp64
 * arithmetic and in the project's fp32 arithmetic spec.  Test
 * infrastructure: compiled by tests/skewopt_spec.py at run time and linked
 * with oracle/build/liboracle.so (orc_word, orc_fast_sigmoid, orc_alpha_line,
 * orc_lane_width; the alias arrays come in through orc_graph).
 *
 * Sample s is unit s of Philox stream 0: slots 0-3 source and target, slots
 * 4 + 2n (index), 5 + 2n (p) negative n of 16 -- the 4 + 2K layout with
 * K = 16.  No draw looks at the table, so the 18 ids are drawn first.  The
 * update works on the table in place, element by element in the reference's
 * order, so rows that coincide (any two of the 18 ids) behave as the
 * reference's vector<double> rows do.
 *
 * The two instances differ only in the macros below:
 *   fp64: f = sequential sum of wv[d] * x[d]; g = (f - xi) / omega;
 *         chain = p / g (0 / 0 at g == 0, as the reference);
 *         gg = sig(-p) * chain / omega, then *= alpha; ve += gg * x;
 *         decay w -= (alpha*0.01) * w; wv += ve / up
 *   fp32: f = lane-order sum (G = orc_lane_width lanes, lane l owns the 16-B
 *         chunks l, l+G, ..: an fmaf chain per lane, then a pairwise tree);
 *         xi, omega rounded to fp32 once; every quotient a / b is the
 *         correctly rounded fp32 quotient (the fp64 quotient of the two fp32
 *         values, rounded once); chain at g == 0 is its limit, 0 for
 *         eta >= 2 and 1 for eta == 1; ve = fmaf(gg, x, ve);
 *         decay w = fmaf(-r, w, w), r = alpha * 0.01f; wv += ve / (float)up
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "smore_oracle.h"

#define SKEW_NEG 16

static inline uint32_t draw_index(uint32_t k, uint64_t n) { return (uint32_t)(((uint64_t)k * n) >> 32); }
/* SourceSample src/proNet.cpp:647-657 (p, then index) */
static int32_t source_sample(const orc_graph* g, uint32_t kp, uint32_t ki) {
    uint32_t i = draw_index(ki, (uint64_t)g->V);
    return kp < g->vthr[i] ? (int32_t)i : g->valias[i];
}
/* TargetSample src/proNet.cpp:671-683 (no out-edge: -1) */
static int32_t target_sample(const orc_graph* g, int32_t v, uint32_t kp, uint32_t ki) {
    int64_t off = g->offsets[v], br = g->offsets[v + 1] - off;
    if (br == 0) return -1;
    int64_t i = off + draw_index(ki, (uint64_t)br);
    return kp < g->cthr[i] ? g->targets[i] : g->calias[i];
}
/* NegativeSample src/proNet.cpp:623-633 (index FIRST, then p) */
static int32_t negative_sample(const orc_graph* g, uint32_t ki, uint32_t kp) {
    uint32_t i = draw_index(ki, (uint64_t)g->V);
    return kp < g->nthr[i] ? (int32_t)i : g->nalias[i];
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

/* the decision trace's code of fastSigmoid(x): the table index, 1001 / 1002
 * for the x < -8 / x > 8 ends (src/proNet.cpp:62-71) */
static int sig_code(double x) {
    if (x < -8.0) return 1001;
    if (x > 8.0) return 1002;
    return (int)((x + 8.0) * 1000 / 8.0 / 2);
}

/* the rule.  T: V rows of `d` REALs (fp32: d = dpad, padding zero), or NULL:
 * the draws only.  Samples [begin, end).  rec: 18 ids {v, i, j_0..j_15} per
 * sample (i < 0: a source without out-edge).  trace: 16 per sample, -1 =
 * gated (g > 2) or sample not run, otherwise the sigmoid code (sig_code).
 * kind: 16 per sample, 0 gated / not run, 1 clamped, 2 interior.  *gmin = min
 * |g| over every negative of the run before gate and clamp (fp64 value).
 * counts[0] += gates passed, counts[1] += samples that updated.  stop >= 0: the
 * run ends at its negative number `stop` (counted over the negatives of the
 * samples that ran), after that negative's g is computed and before the gate
 * acts, with *gstop = g; the table is as that negative found it.  Returns the
 * samples whose source had no out-edge (smore_skipped). */
#define SKEW_SPEC(NAME, REAL, DOT, SIG, CVT, QUOT, CHAIN0, DECAY, ACC, DIVUP)                                 \
    int NAME(const orc_graph* g, REAL* T, int d, double alpha0, double xi_, double omega_, int eta,          \
             uint64_t total, uint64_t begin, uint64_t end, uint64_t seed, int32_t* rec, int16_t* trace,      \
             uint8_t* kind, double* gmin, uint64_t* counts, int64_t stop, double* gstop) {                   \
        REAL* x = (REAL*)malloc(sizeof(REAL) * (size_t)(d > 0 ? d : 1) * 3);                                 \
        REAL *ce = x + d, *ve = x + 2 * d;                                                                   \
        const REAL xi = CVT(xi_), omega = CVT(omega_);                                                       \
        int32_t own[2 + SKEW_NEG];                                                                           \
        int skipped = 0;                                                                                     \
        double gm = INFINITY;                                                                                \
        int64_t gi = 0;                                                                                      \
        for (uint64_t s = begin; s < end; ++s) {                                                             \
            int32_t* r = rec ? rec + (s - begin) * (uint64_t)(2 + SKEW_NEG) : own;                           \
            r[0] = source_sample(g, orc_word(seed, 0, s, 0), orc_word(seed, 0, s, 1));                       \
            r[1] = target_sample(g, r[0], orc_word(seed, 0, s, 2), orc_word(seed, 0, s, 3));                 \
            for (int n = 0; n < SKEW_NEG; ++n) {                                                             \
                r[2 + n] = negative_sample(g, orc_word(seed, 0, s, 4 + 2 * n), orc_word(seed, 0, s, 5 + 2 * n)); \
                if (trace) trace[(s - begin) * SKEW_NEG + n] = -1;                                           \
                if (kind) kind[(s - begin) * SKEW_NEG + n] = 0;                                              \
            }                                                                                                \
            if (r[1] < 0) { skipped++; continue; }                                                           \
            if (!T) continue;                                                                                \
            const REAL alpha = (REAL)orc_alpha_line(s, alpha0, total);                                       \
            const REAL rd = alpha * (REAL)0.01;                                                              \
            REAL* wv = T + (int64_t)r[0] * d;                                                                \
            REAL* wi = T + (int64_t)r[1] * d;                                                                \
            int up = 0;                                                                                      \
            for (int k = 0; k < d; ++k) ve[k] = (REAL)0.0;                                                   \
            for (int n = 0; n < SKEW_NEG; ++n) {                                                             \
                REAL* wj = T + (int64_t)r[2 + n] * d;                                                        \
                for (int k = 0; k < d; ++k) x[k] = wi[k] - wj[k];                                            \
                const REAL f = DOT(wv, x, d);                                                                \
                REAL gq = QUOT(f - xi, omega);                                                               \
                if (gi++ == stop) {                                                                          \
                    if (gstop) *gstop = (double)gq;                                                          \
                    goto done;                                                                               \
                }                                                                                            \
                if (fabs((double)gq) < gm) gm = fabs((double)gq);                                            \
                if (gq > (REAL)2.0) continue;                                                                \
                int kd = 2;                                                                                  \
                if (gq < (REAL)-2.0) { gq = (REAL)-2.0; kd = 1; }                                            \
                REAL p = (REAL)1.0;                                                                          \
                for (int e = 0; e < eta; ++e) p = p * gq;                                                    \
                const REAL chain = CHAIN0(p, gq, eta);                                                       \
                REAL gg = SIG(p) * chain;                                                                    \
                gg = QUOT(gg, omega);                                                                        \
                gg = gg * alpha;                                                                             \
                if (trace) trace[(s - begin) * SKEW_NEG + n] = (int16_t)sig_code(-(double)p);                \
                if (kind) kind[(s - begin) * SKEW_NEG + n] = (uint8_t)kd;                                    \
                for (int k = 0; k < d; ++k) ve[k] = ACC(gg, x[k], ve[k]);                                    \
                for (int k = 0; k < d; ++k) ce[k] = ACC(gg, wv[k], (REAL)0.0);                               \
                for (int k = 0; k < d; ++k) {                                                                \
                    wi[k] = DECAY(rd, wi[k]);                                                                \
                    wj[k] = DECAY(rd, wj[k]);                                                                \
                    wi[k] = wi[k] + ce[k];                                                                   \
                    wj[k] = wj[k] - ce[k];                                                                   \
                }                                                                                            \
                up++;                                                                                        \
                if (counts) counts[0]++;                                                                     \
            }                                                                                                \
            if (up) {                                                                                        \
                for (int k = 0; k < d; ++k) {                                                                \
                    wv[k] = DECAY(rd, wv[k]);                                                                \
                    wv[k] = wv[k] + DIVUP(ve[k], up);                                                        \
                }                                                                                            \
                if (counts) counts[1]++;                                                                     \
            }                                                                                                \
        }                                                                                                    \
    done:                                                                                                    \
        if (gmin) *gmin = gm;                                                                                \
        free(x);                                                                                             \
        return skipped;                                                                                      \
    }

/* fp64: the reference's expressions (g_in_sigmoid / g, fastSigmoid(-1 * p) *
 * chain / omega, then g *= alpha; the decay is w -= alpha*0.01*w; the closing
 * vertex_err[d] / update with update an int) */
#define SIG64(p) orc_fast_sigmoid(-1 * (p))
#define CVT64(a) (a)
#define QUOT64(a, b) ((a) / (b))
#define CHAIN64(p, g, eta) ((p) / (g))
#define DECAY64(r, w) ((w) - (r) * (w))
#define ACC64(g, y, acc) ((acc) + (g) * (y))
#define DIV64(v, up) ((v) / (up))
/* fp32 spec: the sigmoid bucket of the fp32 p is found in fp64 (as the other
 * rules do), its table entry rounded to fp32 */
#define SIG32(p) ((float)orc_fast_sigmoid((double)(-(p))))
#define CVT32(a) ((float)(a))
#define QUOT32(a, b) ((float)((double)(a) / (double)(b)))
#define CHAIN32(p, g, eta) ((g) == 0.0f ? ((eta) >= 2 ? 0.0f : 1.0f) : QUOT32(p, g))
#define DECAY32(r, w) fmaf(-(r), (w), (w))
#define ACC32(g, y, acc) fmaf((g), (y), (acc))
#define DIV32(v, up) QUOT32(v, (float)(up))

SKEW_SPEC(skewopt_spec_f64, double, dot_f64, SIG64, CVT64, QUOT64, CHAIN64, DECAY64, ACC64, DIV64)
SKEW_SPEC(skewopt_spec_f32, float, dot_f32, SIG32, CVT32, QUOT32, CHAIN32, DECAY32, ACC32, DIV32)

/* warp_spec.c -- the WARP rule (WARP::Train, src/model/WARP.cpp:85-91, with
 * proNet::UpdateWARPPair, src/proNet.cpp:1353-1403) written once and
 * instantiated twice: in the reference's fp64 arithmetic and in the project's
 * fp32 arithmetic spec (DESIGN.md "WARP").  Test infrastructure: compiled by
 * tests/test_warp_cpu.py / test_gpu_warp.py at run time and linked with
 * oracle/build/liboracle.so (orc_word, orc_fast_sigmoid, orc_alpha_line,
 * orc_lane_width; the alias arrays come in through orc_graph).
 *
 * Sample s is unit s of Philox stream 0 read as a prefix: slots 0-3 source
 * and target, slots 4 + 2n (index), 5 + 2n (p) the negative of trial n.
 * The update works on the table in place, element by element in the
 * reference's order, so rows that coincide (two of v, i, j equal) behave as
 * the reference's vector<double> rows do.
 *
 * The two instances differ only in the macros below:
 *   fp64: f = sequential sum of wv[d] * x[d]; decay w -= (alpha*0.0025) * w
 *   fp32: f = lane-order sum (G = orc_lane_width lanes, lane l owns the 16-B
 *         chunks l, l+G, ..: an fmaf chain per lane, then a pairwise tree);
 *         decay w = fmaf(-r, w, w), r = alpha * 0.0025f
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "smore_oracle.h"

#define WARP_TRIALS 32

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

/* the rule.  T: V rows of `d` REALs (fp32: d = dpad, padding zero).  Samples
 * [begin, end); ntrials[s - begin] = trials executed (0: source without
 * out-edge), *margin = min |f - 1| over every trial of the run (fp64 value),
 * counts[0] += trials, counts[1] += samples that updated.  Returns skipped. */
#define WARP_SPEC(NAME, REAL, DOT, SIG, RATE, DECAY, ACC0)                                                  \
    int NAME(const orc_graph* g, REAL* T, int d, double alpha0, uint64_t total, uint64_t begin,             \
             uint64_t end, uint64_t seed, int32_t* ntrials, double* margin, uint64_t* counts) {             \
        REAL* x = (REAL*)malloc(sizeof(REAL) * (size_t)d * 3);                                              \
        REAL *ce = x + d, *ve = x + 2 * d;                                                                  \
        int skipped = 0;                                                                                    \
        double mg = INFINITY;                                                                               \
        for (uint64_t s = begin; s < end; ++s) {                                                            \
            int32_t v = source_sample(g, orc_word(seed, 0, s, 0), orc_word(seed, 0, s, 1));                 \
            int32_t i = target_sample(g, v, orc_word(seed, 0, s, 2), orc_word(seed, 0, s, 3));              \
            if (ntrials) ntrials[s - begin] = 0;                                                            \
            if (i < 0) { skipped++; continue; }                                                             \
            const REAL alpha = (REAL)orc_alpha_line(s, alpha0, total);                                      \
            REAL* wv = T + (int64_t)v * d;                                                                  \
            REAL* wi = T + (int64_t)i * d;                                                                  \
            int n;                                                                                          \
            for (n = 0; n < WARP_TRIALS; ++n) {                                                             \
                int32_t j = negative_sample(g, orc_word(seed, 0, s, 4 + 2 * n), orc_word(seed, 0, s, 5 + 2 * n)); \
                REAL* wj = T + (int64_t)j * d;                                                              \
                for (int k = 0; k < d; ++k) x[k] = wi[k] - wj[k];                                           \
                const REAL f = DOT(wv, x, d);                                                               \
                if (fabs((double)f - 1.0) < mg) mg = fabs((double)f - 1.0);                                 \
                if (counts) counts[0]++;                                                                    \
                if (f < (REAL)1.0) {                                                                        \
                    const REAL gg = SIG(f) * alpha;                                                         \
                    const REAL r = RATE(alpha);                                                             \
                    for (int k = 0; k < d; ++k) { ve[k] = ACC0(gg, x[k]); }                                 \
                    for (int k = 0; k < d; ++k) { ce[k] = ACC0(gg, wv[k]); }                                \
                    for (int k = 0; k < d; ++k) {                                                           \
                        wi[k] = DECAY(r, wi[k]);                                                            \
                        wj[k] = DECAY(r, wj[k]);                                                            \
                        wv[k] = DECAY(r, wv[k]);                                                            \
                        wi[k] = wi[k] + ce[k];                                                              \
                        wj[k] = wj[k] - ce[k];                                                              \
                        wv[k] = wv[k] + ve[k];                                                              \
                    }                                                                                       \
                    if (counts) counts[1]++;                                                                \
                    n++;                                                                                    \
                    break;                                                                                  \
                }                                                                                           \
            }                                                                                               \
            if (ntrials) ntrials[s - begin] = n;                                                            \
        }                                                                                                   \
        if (margin) *margin = mg;                                                                           \
        free(x);                                                                                            \
        return skipped;                                                                                     \
    }

/* fp64: Opt_BPRSGD (src/proNet.cpp:1053-1068) adds g * x to a zeroed error
 * vector; the decay is w -= alpha*0.0025*w */
#define SIG64(f) orc_fast_sigmoid(0.0 - (f))
#define RATE64(a) ((a) * 0.0025)
#define DECAY64(r, w) ((w) - (r) * (w))
#define ACC64(g, y) (0.0 + (g) * (y))
/* fp32 spec: the sigmoid bucket of the fp32 dot is found in fp64 (as the
 * other rules do), its table entry rounded to fp32 */
#define SIG32(f) ((float)orc_fast_sigmoid((double)(-(f))))
#define RATE32(a) ((a) * 0.0025f)
#define DECAY32(r, w) fmaf(-(r), (w), (w))
#define ACC32(g, y) fmaf((g), (y), 0.0f)

WARP_SPEC(warp_spec_f64, double, dot_f64, SIG64, RATE64, DECAY64, ACC64)
WARP_SPEC(warp_spec_f32, float, dot_f32, SIG32, RATE32, DECAY32, ACC32)

/* hoprec_spec.c -- the HOP-REC rule (HBPR::Train, src/model/HBPR.cpp:94-114,
 * with proNet::UpdateFBPRPair, src/proNet.cpp:1458-1515, and Opt_FBPRSGD,
 * :1014-1031) written once and instantiated twice: in the reference's fp64
 * arithmetic and in the project's fp32 arithmetic spec.  Test
 * infrastructure: compiled by tests/hoprec_spec.py at run time and linked with
 * oracle/build/liboracle.so (orc_word, orc_fast_sigmoid, orc_alpha_line,
 * orc_lane_width; the alias arrays come in through orc_graph).
 *
 * Sample s is unit s of Philox stream 0, its slots consumed consecutively in
 * the order of the reference's random_gen calls: source attempts 2 slots each
 * (p, index) until field[v] == 0; TargetSample 2 (p, index; a vertex without
 * out-edge takes none and returns -1); per step w > 1 two more TargetSample;
 * NegativeSample attempts 2 each (index, p) until field[j] == field[i]; the
 * in-rule negatives j1..j4 one slot per attempt, a uniform index.  A
 * rejection loop gives up after 2^16 attempts: the sample stops at that step.
 * The draws never look at the tables, so they are made first (hoprec_draw)
 * and the steps run on the record.
 *
 * The update works on the table in place, element by element in the
 * reference's order, so rows that coincide behave as the reference's
 * vector<double> rows do.
 *
 * The two instances differ only in the macros below:
 *   fp64: rate = alpha / w, margin = 1.0 / w; f = sequential sum of wv[d] * x[d];
 *         ve += g * x; decay w -= (rate*0.0025) * w; wv += ve / up
 *   fp32: rate = (float)((double)alpha / w) -- the fp64 quotient of the fp32
 *         alpha, rounded once -- margin = (float)(1.0 / w); f = lane-order sum
 *         (G = orc_lane_width lanes, lane l owns the 16-B chunks l, l+G, ..:
 *         an fmaf chain per lane, then a pairwise tree); ve = fmaf(g, x, ve);
 *         decay w = fmaf(-r, w, w), r = rate * 0.0025f (0.025f for v);
 *         wv += ve / (float)up
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "smore_oracle.h"

#define HOPREC_NEG 5
#define HOPREC_ATTEMPTS (1u << 16)

static inline uint32_t draw_index(uint32_t k, uint64_t n) { return (uint32_t)(((uint64_t)k * n) >> 32); }
/* SourceSample src/proNet.cpp:647-657 (p, then index) */
static int32_t source_sample(const orc_graph* g, uint32_t kp, uint32_t ki) {
    uint32_t i = draw_index(ki, (uint64_t)g->V);
    return kp < g->vthr[i] ? (int32_t)i : g->valias[i];
}
/* NegativeSample src/proNet.cpp:623-633 (index FIRST, then p) */
static int32_t negative_sample(const orc_graph* g, uint32_t ki, uint32_t kp) {
    uint32_t i = draw_index(ki, (uint64_t)g->V);
    return kp < g->nthr[i] ? (int32_t)i : g->nalias[i];
}

typedef struct {
    const orc_graph* g;
    uint64_t seed, unit;
    uint32_t slot;
} unit_words;
static uint32_t next_word(unit_words* u) { return orc_word(u->seed, 0, u->unit, u->slot++); }
/* TargetSample src/proNet.cpp:671-683 (no out-edge: -1 before any draw; p, then index) */
static int32_t target_sample(unit_words* u, int32_t v) {
    const orc_graph* g = u->g;
    int64_t off = g->offsets[v], br = g->offsets[v + 1] - off;
    if (br == 0) return -1;
    uint32_t kp = next_word(u), ki = next_word(u);
    int64_t i = off + draw_index(ki, (uint64_t)br);
    return kp < g->cthr[i] ? g->targets[i] : g->calias[i];
}

int hoprec_width(int steps) { return (1 + (1 + HOPREC_NEG) * steps + 3) & ~3; }

/* the draws of sample s into rec (hoprec_width(steps) words, -1 from the step
 * the sample stopped at); returns the steps drawn, *slots the slots consumed */
int hoprec_draw(const orc_graph* g, const int32_t* field, uint64_t seed, uint64_t s, int steps, int32_t* rec,
                uint32_t* slots) {
    const int RW = hoprec_width(steps);
    unit_words u = {g, seed, s, 0};
    int done = 0;
    for (int k = 0; k < RW; ++k) rec[k] = -1;
    int32_t v = -1, i = -1;
    uint32_t a;
    for (a = 0; a < HOPREC_ATTEMPTS; ++a) {
        uint32_t kp = next_word(&u), ki = next_word(&u);
        v = source_sample(g, kp, ki);
        if (field[v] == 0) break;
    }
    if (a < HOPREC_ATTEMPTS) {
        rec[0] = v;
        i = target_sample(&u, v);
        for (int w = 1; w <= steps && i >= 0; ++w) {
            if (w > 1) {
                i = target_sample(&u, i);
                if (i >= 0) i = target_sample(&u, i);
                if (i < 0) break;
            }
            int32_t j[HOPREC_NEG];
            int ok = 1;
            for (int n = 0; n < HOPREC_NEG && ok; ++n) {
                for (a = 0; a < HOPREC_ATTEMPTS; ++a) {
                    if (n == 0) {
                        uint32_t ki = next_word(&u), kp = next_word(&u);
                        j[n] = negative_sample(g, ki, kp);
                    } else {
                        j[n] = (int32_t)draw_index(next_word(&u), (uint64_t)g->V);
                    }
                    if (field[j[n]] == field[i]) break;
                }
                ok = a < HOPREC_ATTEMPTS;
            }
            if (!ok) break;
            int32_t* o = rec + 1 + (1 + HOPREC_NEG) * (w - 1);
            o[0] = i;
            for (int n = 0; n < HOPREC_NEG; ++n) o[1 + n] = j[n];
            done = w;
        }
    }
    if (slots) *slots = u.slot;
    return done;
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

/* the rule.  T: V rows of `d` REALs (fp32: d = dpad, padding zero), or NULL:
 * the draws only.  Samples [begin, end).  rec: hoprec_width(steps) words per
 * sample, slots: slots consumed per sample, pass: 5 * steps gate bits per
 * sample (1 = the negative updated; 0 also for a step not run) -- each may be
 * NULL.  *margin = min |f - margin_w| over every gate of the run (fp64 value),
 * counts[0] += gates tested, counts[1] += gates passed.  stop >= 0: the run
 * ends at its gate number `stop` (counted over the run's gates), after that
 * gate's f is computed and before it acts, with *fstop = f; the table is as
 * the gate found it.  Returns the samples that stopped early (smore_skipped). */
#define HOPREC_SPEC(NAME, REAL, DOT, SIG, RATEW, MARGINW, DECAY, ACC, DIVUP)                                  \
    int NAME(const orc_graph* g, const int32_t* field, REAL* T, int d, int steps, double alpha0,            \
             uint64_t total, uint64_t begin, uint64_t end, uint64_t seed, int32_t* rec, uint32_t* slots,     \
             uint8_t* pass, double* margin, uint64_t* counts, int64_t stop, double* fstop) {                 \
        const int RW = hoprec_width(steps);                                                                  \
        REAL* x = (REAL*)malloc(sizeof(REAL) * (size_t)(d > 0 ? d : 1) * 3);                                 \
        REAL *ce = x + d, *ve = x + 2 * d;                                                                   \
        int32_t own[64];                                                                                     \
        int skipped = 0;                                                                                     \
        double mg = INFINITY;                                                                                \
        int64_t gi = 0;                                                                                      \
        for (uint64_t s = begin; s < end; ++s) {                                                             \
            int32_t* r = rec ? rec + (s - begin) * (uint64_t)RW : own;                                       \
            uint32_t sl;                                                                                     \
            const int done = hoprec_draw(g, field, seed, s, steps, r, &sl);                                  \
            if (slots) slots[s - begin] = sl;                                                                \
            if (pass)                                                                                        \
                for (int k = 0; k < HOPREC_NEG * steps; ++k) pass[(s - begin) * (uint64_t)(HOPREC_NEG * steps) + k] = 0; \
            if (done < steps) skipped++;                                                                     \
            if (!T) continue;                                                                                \
            const REAL alpha = (REAL)orc_alpha_line(s, alpha0, total);                                       \
            REAL* wv = T + (int64_t)r[0] * d;                                                                \
            for (int w = 1; w <= done; ++w) {                                                                \
                const int32_t* o = r + 1 + (1 + HOPREC_NEG) * (w - 1);                                       \
                const REAL rate = RATEW(alpha, w), mw = MARGINW(w);                                          \
                const REAL rd = rate * (REAL)0.0025, rdv = rate * (REAL)0.025;                               \
                REAL* wi = T + (int64_t)o[0] * d;                                                            \
                int up = 0;                                                                                  \
                for (int k = 0; k < d; ++k) ve[k] = (REAL)0.0;                                               \
                for (int n = 0; n < HOPREC_NEG; ++n) {                                                       \
                    REAL* wj = T + (int64_t)o[1 + n] * d;                                                    \
                    for (int k = 0; k < d; ++k) x[k] = wi[k] - wj[k];                                        \
                    const REAL f = DOT(wv, x, d);                                                            \
                    if (gi++ == stop) {                                                                      \
                        if (fstop) *fstop = (double)f;                                                       \
                        goto done;                                                                           \
                    }                                                                                        \
                    if (fabs((double)f - (double)mw) < mg) mg = fabs((double)f - (double)mw);                \
                    if (counts) counts[0]++;                                                                 \
                    if (f > mw) continue;                                                                    \
                    const REAL gg = SIG(f) * rate;                                                           \
                    for (int k = 0; k < d; ++k) ve[k] = ACC(gg, x[k], ve[k]);                                \
                    for (int k = 0; k < d; ++k) ce[k] = ACC(gg, wv[k], (REAL)0.0);                           \
                    for (int k = 0; k < d; ++k) {                                                            \
                        wi[k] = DECAY(rd, wi[k]);                                                            \
                        wj[k] = DECAY(rd, wj[k]);                                                            \
                        wi[k] = wi[k] + ce[k];                                                               \
                        wj[k] = wj[k] - ce[k];                                                               \
                    }                                                                                        \
                    up++;                                                                                    \
                    if (counts) counts[1]++;                                                                 \
                    if (pass) pass[(s - begin) * (uint64_t)(HOPREC_NEG * steps) + HOPREC_NEG * (w - 1) + n] = 1; \
                }                                                                                            \
                if (up)                                                                                      \
                    for (int k = 0; k < d; ++k) {                                                            \
                        wv[k] = DECAY(rdv, wv[k]);                                                           \
                        wv[k] = wv[k] + DIVUP(ve[k], up);                                                    \
                    }                                                                                        \
            }                                                                                                \
        }                                                                                                    \
    done:                                                                                                    \
        if (margin) *margin = mg;                                                                            \
        free(x);                                                                                             \
        return skipped;                                                                                      \
    }

/* fp64: the reference's expressions (HBPR.cpp:113 _alpha/w, margin/w; the
 * decay is w -= rate*0.0025*w; vertex_err[d]/up with up a double) */
#define SIG64(f) orc_fast_sigmoid(0.0 - (f))
#define RATE64(a, w) ((a) / (w))
#define MARGIN64(w) (1.0 / (w))
#define DECAY64(r, w) ((w) - (r) * (w))
#define ACC64(g, y, acc) ((acc) + (g) * (y))
#define DIV64(v, up) ((v) / (double)(up))
/* fp32 spec: the sigmoid bucket of the fp32 dot is found in fp64 (as the
 * other rules do), its table entry rounded to fp32 */
#define SIG32(f) ((float)orc_fast_sigmoid((double)(-(f))))
#define RATE32(a, w) ((float)((double)(a) / (double)(w)))
#define MARGIN32(w) ((float)(1.0 / (double)(w)))
#define DECAY32(r, w) fmaf(-(r), (w), (w))
#define ACC32(g, y, acc) fmaf((g), (y), (acc))
#define DIV32(v, up) ((v) / (float)(up))

HOPREC_SPEC(hoprec_spec_f64, double, dot_f64, SIG64, RATE64, MARGIN64, DECAY64, ACC64, DIV64)
HOPREC_SPEC(hoprec_spec_f32, float, dot_f32, SIG32, RATE32, MARGIN32, DECAY32, ACC32, DIV32)

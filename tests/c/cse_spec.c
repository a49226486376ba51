/* cse_spec.c -- the CSE rule (NEMF::Train, src/model/NEMF.cpp:87-149, and
 * NERANK::Train, src/model/NERANK.cpp:87-148, with proNet::UpdateBatchCommunity,
 * src/proNet.cpp:3139-3178, Opt_SigmoidRegSGD :1332-1351, UpdateFactorizedPair
 * :2591-2614, Opt_SGD :991-1012, UpdateUIPair :2616-2663 and Opt_BPRSGD
 * :1053-1068) written once and instantiated twice: in the reference's fp64
 * arithmetic and in the project's fp32 arithmetic spec.  Test
 * infrastructure: compiled by tests/cse_spec.py at run time and linked with
 * oracle/build/liboracle.so.
 *
 * Four tables WU, WI, CU, CI.  Sample s is unit s of Philox stream 0, its slots
 * consumed consecutively in the order of the reference's random_gen calls:
 * source attempts 2 slots each (p, index) until field[v] == 0; c =
 * TargetSample(v) 2 (p, index; a vertex without out-edge takes none and
 * returns -1); pass A (vertex c in WI, contexts in CI, the walk starts at v)
 * and pass B (vertex v in WU, contexts in CU, the walk starts at c): per step
 * s > 0 one TargetSample of the previous context, then five NegativeSample
 * (index, p); then the direct term's negatives: nemf five NegativeSample,
 * nerank sixteen uniform indices, one slot per attempt, each repeated until
 * field[j] == field[c] (at most 2^16 attempts).  The reference stops drawing
 * at the nerank negative that passes; the draws here go on to the sixteenth,
 * and dslot[n] keeps the slots consumed up to negative n so that the slots the
 * reference consumed can be told.  None of the draws looks at the tables, so
 * they are made first (cse_draw) and the rule runs on the record
 *   {v, c, A: n00..n04, then per step s >= 1 ctx_s, ns0..ns4; B: the same; D}
 * 12 steps + D words (D = 5 or 16), padded to a multiple of 4; -1 from where
 * a pass stopped.
 *
 * The update works on the tables in place, element by element in the
 * reference's order, so rows that coincide behave as the reference's
 * vector<double> rows do.
 *
 * The two instances differ only in the macros below:
 *   fp64: the reference's expressions as written
 *   fp32: rate_AB = (float)((double)alpha * 0.05); f = lane-order sum (G =
 *         orc_lane_width lanes, an fmaf chain per lane, then a pairwise tree);
 *         passes: a = rate_AB * (label - sig(f)), back = fmaf(a, ctx, back),
 *         ctx = fmaf(a, w, ctx), w = w + back;
 *         nemf: a = alpha * (label - f), r = alpha * 0.025f, back = fmaf(-r, w,
 *         fmaf(a, ctx, back)), ctx = fmaf(a, w, fmaf(-r, ctx, ctx));
 *         nerank: gate f < 1.0f, gg = sig(-f) * alpha, ve = gg * x, ce = gg * wu,
 *         decays fmaf(-r, w, w), then + ce, - ce, + ve.
 *   The sigmoid bucket of the fp32 f is found in fp64, its entry rounded to fp32.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "smore_oracle.h"

#define CSE_NEG 5
#define CSE_RANK_NEG 16
#define CSE_ATTEMPTS (1u << 16)

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
/* NegativeSample src/proNet.cpp:623-633 (index FIRST, then p) */
static int32_t negative_sample(unit_words* u) {
    const orc_graph* g = u->g;
    uint32_t ki = next_word(u), kp = next_word(u);
    uint32_t i = draw_index(ki, (uint64_t)g->V);
    return kp < g->nthr[i] ? (int32_t)i : g->nalias[i];
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

int cse_dneg(int rank) { return rank ? CSE_RANK_NEG : CSE_NEG; }
int cse_width(int steps, int rank) { return (12 * steps + cse_dneg(rank) + 3) & ~3; }

/* the draws of sample s into rec (cse_width words).  Returns 0: complete, 1: a
 * pass or the direct term stopped early (the rest runs), 2: no sample (no
 * field-0 source within the attempts, or c == -1).  dslot (16 words or NULL):
 * slots consumed up to and including direct negative n. */
int cse_draw(const orc_graph* g, const int32_t* field, uint64_t seed, uint64_t s, int steps, int rank, int32_t* rec,
             uint32_t* slots, uint32_t* dslot) {
    const int RW = cse_width(steps, rank), D = cse_dneg(rank);
    unit_words u = {g, seed, s, 0};
    int early = 0;
    for (int k = 0; k < RW; ++k) rec[k] = -1;
    if (dslot)
        for (int n = 0; n < CSE_RANK_NEG; ++n) dslot[n] = 0;
    int32_t v = -1, c = -1;
    uint32_t a;
    for (a = 0; a < CSE_ATTEMPTS; ++a) {
        v = source_sample(&u);
        if (field[v] == 0) break;
    }
    if (a < CSE_ATTEMPTS) {
        rec[0] = v;
        c = target_sample(&u, v);
    }
    if (c < 0) {
        if (slots) *slots = u.slot;
        return 2;
    }
    rec[1] = c;
    for (int p = 0; p < 2; ++p) {
        int32_t* o = rec + 2 + p * (6 * steps - 1);
        int32_t ctx = p == 0 ? v : c;
        for (int st = 0; st < steps; ++st) {
            int32_t* q = o;
            if (st) {
                ctx = target_sample(&u, ctx);
                if (ctx < 0) {
                    early = 1;
                    break;
                }
                q = o + CSE_NEG + 6 * (st - 1);
                *q++ = ctx;
            }
            for (int n = 0; n < CSE_NEG; ++n) q[n] = negative_sample(&u);
        }
    }
    int32_t* dn = rec + 12 * steps;
    for (int n = 0; n < D; ++n) {
        if (!rank) {
            dn[n] = negative_sample(&u);
        } else {
            int32_t j = -1;
            for (a = 0; a < CSE_ATTEMPTS; ++a) {
                j = (int32_t)draw_index(next_word(&u), (uint64_t)g->V);
                if (field[j] == field[c]) break;
            }
            if (a == CSE_ATTEMPTS) {
                early = 1;
                break;
            }
            dn[n] = j;
        }
        if (dslot) dslot[n] = u.slot;
    }
    if (slots) *slots = u.slot;
    return early;
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

/* the rule.  WU, WI, CU, CI: V rows of `d` REALs each (fp32: d = dpad, padding
 * zero); WU == NULL: the draws only.  Samples [begin, end).  Per sample (each
 * array may be NULL): rec cse_width words; slots: slots the draws consumed;
 * used: slots the reference consumes (nerank stops drawing at its break);
 * pass: nerank, the index of the negative that passed, -1 none; nemf 0; -2 no
 * sample.  *margin = min |f - 1| over the nerank gates of the run (fp64
 * value); counts[0] += nerank gates tested, counts[1] += nerank updates.
 * stop >= 0: the run ends at its nerank gate number `stop` (counted over the
 * run), after that gate's f is computed and before it acts, *fstop = f.
 * Returns the samples counted as skipped. */
#define CSE_SPEC(NAME, REAL, DOT, SIGP, SIGN, RATEAB, PASSUPD, SGDUPD, DECAY, MUL)                                  \
    int NAME(const orc_graph* g, const int32_t* field, REAL* WU, REAL* WI, REAL* CU, REAL* CI, int d, int steps,   \
             int rank, double alpha0, uint64_t total, uint64_t begin, uint64_t end, uint64_t seed, int32_t* rec,   \
             uint32_t* slots, uint32_t* used, int32_t* pass, double* margin, uint64_t* counts, int64_t stop,       \
             double* fstop) {                                                                                      \
        const int RW = cse_width(steps, rank), D = cse_dneg(rank);                                                 \
        REAL* back = (REAL*)malloc(sizeof(REAL) * (size_t)(d > 0 ? d : 1) * 4);                                    \
        REAL *x = back + d, *ce = back + 2 * d, *ve = back + 3 * d;                                                \
        int32_t own[160];                                                                                          \
        uint32_t dslot[CSE_RANK_NEG];                                                                              \
        int skipped = 0;                                                                                           \
        double mg = INFINITY;                                                                                      \
        int64_t gi = 0;                                                                                            \
        for (uint64_t s = begin; s < end; ++s) {                                                                   \
            int32_t* r = rec ? rec + (s - begin) * (uint64_t)RW : own;                                             \
            uint32_t sl;                                                                                           \
            const int st = cse_draw(g, field, seed, s, steps, rank, r, &sl, dslot);                                \
            if (slots) slots[s - begin] = sl;                                                                      \
            if (used) used[s - begin] = sl;                                                                        \
            if (pass) pass[s - begin] = st == 2 ? -2 : rank ? -1 : 0;                                              \
            if (st) skipped++;                                                                                     \
            if (st == 2 || !WU) continue;                                                                          \
            const REAL alpha = (REAL)orc_alpha_line(s, alpha0, total);                                             \
            const REAL rab = RATEAB(alpha);                                                                        \
            const int32_t v = r[0], c = r[1];                                                                      \
            for (int p = 0; p < 2; ++p) {                                                                          \
                REAL* w = p == 0 ? WI + (int64_t)c * d : WU + (int64_t)v * d;                                      \
                REAL* Cx = p == 0 ? CI : CU;                                                                       \
                const int32_t* o = r + 2 + p * (6 * steps - 1);                                                    \
                for (int k = 0; k < d; ++k) back[k] = (REAL)0.0;                                                   \
                for (int q = 0; q < steps; ++q) {                                                                  \
                    const int32_t* ids = q ? o + CSE_NEG + 6 * (q - 1) : o - 1;                                    \
                    const int32_t ctx = q ? ids[0] : (p == 0 ? v : c);                                             \
                    if (ctx < 0) break;                                                                            \
                    for (int n = 0; n <= CSE_NEG; ++n) {                                                           \
                        REAL* cr = Cx + (int64_t)(n ? ids[n] : ctx) * d;                                           \
                        const REAL gl = (n ? (REAL)0.0 : (REAL)1.0) - SIGP(DOT(w, cr, d));                         \
                        PASSUPD(rab, gl, w, cr, back, d)                                                           \
                    }                                                                                              \
                    for (int k = 0; k < d; ++k) {                                                                  \
                        w[k] = w[k] + back[k];                                                                     \
                        back[k] = (REAL)0.0;                                                                       \
                    }                                                                                              \
                }                                                                                                  \
            }                                                                                                      \
            REAL* wu = WU + (int64_t)v * d;                                                                        \
            REAL* wc = WI + (int64_t)c * d;                                                                        \
            const int32_t* dn = r + 12 * steps;                                                                    \
            if (!rank) {                                                                                           \
                const REAL reg = (REAL)0.025;                                                                      \
                for (int k = 0; k < d; ++k) back[k] = (REAL)0.0;                                                   \
                for (int n = 0; n <= CSE_NEG; ++n) {                                                               \
                    REAL* cr = n ? WI + (int64_t)dn[n - 1] * d : wc;                                               \
                    const REAL gl = (n ? (REAL)-1.0 : (REAL)1.0) - DOT(wu, cr, d);                                 \
                    SGDUPD(alpha, reg, gl, wu, cr, back, d)                                                        \
                }                                                                                                  \
                for (int k = 0; k < d; ++k) wu[k] = wu[k] + back[k];                                               \
                continue;                                                                                          \
            }                                                                                                      \
            for (int n = 0; n < D && dn[n] >= 0; ++n) {                                                            \
                REAL* wj = WI + (int64_t)dn[n] * d;                                                                \
                for (int k = 0; k < d; ++k) x[k] = wc[k] - wj[k];                                                  \
                const REAL f = DOT(wu, x, d);                                                                      \
                if (gi++ == stop) {                                                                                \
                    if (fstop) *fstop = (double)f;                                                                 \
                    goto done;                                                                                     \
                }                                                                                                  \
                if (fabs((double)f - 1.0) < mg) mg = fabs((double)f - 1.0);                                        \
                if (counts) counts[0]++;                                                                           \
                if (!(f < (REAL)1.0)) continue;                                                                    \
                const REAL gg = SIGN(f) * alpha;                                                                   \
                const REAL rr = MUL(alpha, (REAL)0.025);                                                           \
                for (int k = 0; k < d; ++k) ve[k] = MUL(gg, x[k]);                                                 \
                for (int k = 0; k < d; ++k) ce[k] = MUL(gg, wu[k]);                                                \
                for (int k = 0; k < d; ++k) {                                                                      \
                    wc[k] = DECAY(rr, wc[k]);                                                                      \
                    wj[k] = DECAY(rr, wj[k]);                                                                      \
                    wu[k] = DECAY(rr, wu[k]);                                                                      \
                    wc[k] = wc[k] + ce[k];                                                                         \
                    wj[k] = wj[k] - ce[k];                                                                         \
                    wu[k] = wu[k] + ve[k];                                                                         \
                }                                                                                                  \
                if (counts) counts[1]++;                                                                           \
                if (pass) pass[s - begin] = n;                                                                     \
                if (used) used[s - begin] = dslot[n];                                                              \
                break;                                                                                             \
            }                                                                                                      \
        }                                                                                                          \
    done:                                                                                                          \
        if (margin) *margin = mg;                                                                                  \
        free(back);                                                                                                \
        return skipped;                                                                                            \
    }

/* fp64: the reference's expressions.  Opt_SigmoidRegSGD with reg = 0.0 (the
 * products by 0.0 are kept), Opt_SGD with reg = 0.025, both with the context
 * row as its own loss vector: the back-error loop reads the row before the
 * context loop moves it. */
#define SIGP64(f) orc_fast_sigmoid(f)
#define SIGN64(f) orc_fast_sigmoid(0.0 - (f))
#define RATEAB64(a) ((a) * 0.05)
#define PASS64(rate, gl, w, cr, back, d)                                                     \
    for (int k = 0; k < d; ++k) back[k] += (rate) * ((gl) * cr[k] - 0.0 * w[k]);             \
    for (int k = 0; k < d; ++k) cr[k] += (rate) * ((gl) * w[k] - 0.0 * cr[k]);
#define SGD64(al, reg, gl, w, cr, back, d)                                                   \
    for (int k = 0; k < d; ++k) back[k] += (al) * ((gl) * cr[k] - (reg) * w[k]);             \
    for (int k = 0; k < d; ++k) cr[k] += (al) * ((gl) * w[k] - (reg) * cr[k]);
#define DECAY64(r, w) ((w) - (r) * (w))
#define MUL64(a, b) ((a) * (b))

#define SIGP32(f) ((float)orc_fast_sigmoid((double)(f)))
#define SIGN32(f) ((float)orc_fast_sigmoid((double)(-(f))))
#define RATEAB32(a) ((float)((double)(a) * 0.05))
#define PASS32(rate, gl, w, cr, back, d)                                                     \
    {                                                                                        \
        const float a_ = (rate) * (gl);                                                      \
        for (int k = 0; k < d; ++k) back[k] = fmaf(a_, cr[k], back[k]);                      \
        for (int k = 0; k < d; ++k) cr[k] = fmaf(a_, w[k], cr[k]);                           \
    }
#define SGD32(al, reg, gl, w, cr, back, d)                                                   \
    {                                                                                        \
        const float a_ = (al) * (gl), r_ = (al) * (reg);                                     \
        for (int k = 0; k < d; ++k) back[k] = fmaf(-r_, w[k], fmaf(a_, cr[k], back[k]));     \
        for (int k = 0; k < d; ++k) cr[k] = fmaf(a_, w[k], fmaf(-r_, cr[k], cr[k]));         \
    }
#define DECAY32(r, w) fmaf(-(r), (w), (w))
#define MUL32(a, b) ((a) * (b))

CSE_SPEC(cse_spec_f64, double, dot_f64, SIGP64, SIGN64, RATEAB64, PASS64, SGD64, DECAY64, MUL64)
CSE_SPEC(cse_spec_f32, float, dot_f32, SIGP32, SIGN32, RATEAB32, PASS32, SGD32, DECAY32, MUL32)

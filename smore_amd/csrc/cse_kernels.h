// cse_kernels.h -- the CSE update kernel for gfx950 (template): nemf (RANK 0) and
// nerank (RANK 1) on the four tables WU, WI, CU, CI.
//
// NEMF::Train / NERANK::Train (src/model/NEMF.cpp:119-131, NERANK.cpp:119-130) run
// per sample (v a field-0 vertex, c = TargetSample(v)):
//   pass A  UpdateBatchCommunity(WI, CI, vertex c, walk from v) at rate alpha 0.05
//   pass B  UpdateBatchCommunity(WU, CU, vertex v, walk from c) at rate alpha 0.05
//           (src/proNet.cpp:3139-3178, Opt_SigmoidRegSGD :1332-1351): per step the
//           walk's context (label 1) and five negatives (label 0); each context row
//           moves by rate g W[vertex] and adds rate g C[ctx] to the step's back
//           error, which the vertex row takes at the end of the step
//   nemf    UpdateFactorizedPair(WU, WI, v, c) (:2591-2614, Opt_SGD :991-1012): g =
//           label - f without a sigmoid, labels +1 (c) and -1 (five negatives), decay
//           0.025 inside the same expression
//   nerank  UpdateUIPair (:2616-2663): up to sixteen same-field negatives j, f =
//           WU[v] . (WI[c] - WI[j]); the first with f < 1 runs Opt_BPRSGD (:1053-1068),
//           decays the three rows and moves them, then the loop breaks
// Every id comes pre-drawn in the record (train_cse_draw.hip).  DESIGN.md 12d.
//
// One lane group of G lanes per sample (device_common.h row layout).  WU[v] and
// WI[c] stay in registers for the whole sample: pass A's vertex row, pass B's
// vertex row, then both in the direct term.  The passes touch disjoint tables
// (A: WI, CI; B: WU, CU), so step s of A and step s of B are independent: when
// the six context rows of a step are pairwise distinct in both passes the
// twelve are requested together ahead of the first wait and the twelve updates
// run from registers.  When ids coincide within a pass's step that step runs in
// the reference's memory order: every context row is read after the previous
// one was written.  nerank's gates before the one that passes see untouched
// rows, so its sixteen negative rows are gathered eight at a time and gated
// from registers (a negative equal to c is WI[c] as the registers hold it).
#pragma once
#include "hoprec_kernels.h"

namespace smore {

// rate of passes A and B as the fp32 rule takes it (tests/c/cse_spec.c): the fp64 product
// of the fp32 alpha, rounded once
__device__ __forceinline__ float cse_rate_ab(float alpha) { return (float)((double)alpha * 0.05); }

// row q takes nw: a plain store, or (atomic scatter) one add of nw - old
template <int G, int M, int MODE>
__device__ __forceinline__ void cse_put(float* q, const float (&nw)[M], const float (&old)[M], int lane,
                                        const bool (&ev)[M], int dpad) {
    if constexpr (MODE == MODE_ATOMIC) {
        float dl[M];
#pragma unroll
        for (int m = 0; m < M; ++m) dl[m] = nw[m] - old[m];
        atomic_row<G, M>(q, dl, lane, dpad);
    } else {
        st_row<G, M>(q, nw, lane, ev);
    }
}

template <int G, int M>
__device__ __forceinline__ float cse_dot(const float (&a)[M], const float (&b)[M]) {
    float p = 0.0f;
#pragma unroll
    for (int m = 0; m < M; ++m) p = __builtin_fmaf(a[m], b[m], p);
    return group_sum<G>(p);
}

__device__ __forceinline__ bool cse_distinct6(const int32_t (&id)[6]) {
    bool d = true;
#pragma unroll
    for (int n = 1; n < 6; ++n)
#pragma unroll
        for (int k = 0; k < n; ++k) d = d && id[n] != id[k];
    return d;
}

// one Opt_SigmoidRegSGD of vertex row w against context row `row` (label 1 for the
// walk's context, 0 for a negative): nw = the moved context row, back += its share
template <int G, int M>
__device__ __forceinline__ void cse_sig_update(const float (&w)[M], const float (&row)[M], float label, float rab,
                                               const float* s_sig, float (&back)[M], float (&nw)[M]) {
    const float a_ = rab * (label - fast_sigmoid(cse_dot<G, M>(w, row), s_sig));
#pragma unroll
    for (int m = 0; m < M; ++m) {
        back[m] = __builtin_fmaf(a_, row[m], back[m]);
        nw[m] = __builtin_fmaf(a_, w[m], row[m]);
    }
}

// a pass's step on six context rows already in registers (pairwise distinct ids)
template <int G, int M, int MODE>
__device__ __forceinline__ void cse_step_regs(float* Cx, const int32_t (&id)[6], const float (&row)[6][M], float (&w)[M],
                                              float rab, const float* s_sig, int lane, const bool (&ev)[M], int dpad) {
    float back[M];
#pragma unroll
    for (int m = 0; m < M; ++m) back[m] = 0.0f;
#pragma unroll
    for (int n = 0; n < 6; ++n) {
        float nw[M];
        cse_sig_update<G, M>(w, row[n], n ? 0.0f : 1.0f, rab, s_sig, back, nw);
        cse_put<G, M, MODE>(Cx + (int64_t)id[n] * dpad, nw, row[n], lane, ev, dpad);
    }
#pragma unroll
    for (int m = 0; m < M; ++m) w[m] = w[m] + back[m];
}

// a pass's step: six rows in flight together when the ids are distinct, else in the
// reference's memory order (each row read after the previous one was written)
template <int G, int M, int MODE>
__device__ __forceinline__ void cse_step(float* Cx, const int32_t (&id)[6], bool distinct, float (&w)[M], float rab,
                                         const float* s_sig, int lane, const bool (&ev)[M], int dpad) {
    if (distinct) {
        float row[6][M];
#pragma unroll
        for (int n = 0; n < 6; ++n) ld_row_together<G, M>(row[n], Cx + (int64_t)id[n] * dpad, lane, ev);
        cse_step_regs<G, M, MODE>(Cx, id, row, w, rab, s_sig, lane, ev, dpad);
        return;
    }
    float back[M];
#pragma unroll
    for (int m = 0; m < M; ++m) back[m] = 0.0f;
#pragma unroll
    for (int n = 0; n < 6; ++n) {
        float* const q = Cx + (int64_t)id[n] * dpad;
        float row[M], nw[M];
        ld_row<G, M>(row, q, lane, ev);
        cse_sig_update<G, M>(w, row, n ? 0.0f : 1.0f, rab, s_sig, back, nw);
        cse_put<G, M, MODE>(q, nw, row, lane, ev, dpad);
    }
#pragma unroll
    for (int m = 0; m < M; ++m) w[m] = w[m] + back[m];
}

// One sample: record r (cse_width(a.steps, RANK) words) at learning rate alpha.
// tested / updated: the nerank gates this sample evaluated / its update (0 or 1).
template <int G, int M, int MODE, int RANK>
__device__ __forceinline__ void cse_sample(const CseArgs& a, const float* s_sig, int lane, const bool (&ev)[M],
                                           const int32_t* r, float alpha, unsigned& tested, unsigned& updated) {
    const int dpad = a.dpad, S = a.steps;
    const int32_t v = r[0], c = r[1];
    if (v < 0 || c < 0) return;
    float* const WI = a.T[1];
    float* const CU = a.T[2];
    float* const CI = a.T[3];
    float* const qu = a.T[0] + (int64_t)v * dpad;
    float* const qc = WI + (int64_t)c * dpad;
    float wu[M], wc[M], u0[M], c0[M];
    ld_row_together<G, M>(wu, qu, lane, ev);
    ld_row_together<G, M>(wc, qc, lane, ev);
#pragma unroll
    for (int m = 0; m < M; ++m) {
        u0[m] = wu[m];
        c0[m] = wc[m];
    }
    const float rab = cse_rate_ab(alpha);
    const int32_t* const oA = r + 2;
    const int32_t* const oB = r + 2 + (6 * S - 1);
    bool liveA = true, liveB = true;
    for (int st = 0; st < S && (liveA || liveB); ++st) {
        // the step's ids: step 0 walks from v (A) / c (B), later steps read their context
        const int base = st ? CSE_NEG + 6 * (st - 1) : -1;
        int32_t ia[6], ib[6];
#pragma unroll
        for (int n = 0; n < 6; ++n) {
            ia[n] = (st || n) ? oA[base + n] : v;
            ib[n] = (st || n) ? oB[base + n] : c;
        }
        liveA = liveA && ia[0] >= 0;
        liveB = liveB && ib[0] >= 0;
        const bool dA = cse_distinct6(ia), dB = cse_distinct6(ib);
        if (liveA && liveB && dA && dB) {
            // twelve gathers in flight, then the twelve updates from registers
            float ra[6][M], rb[6][M];
#pragma unroll
            for (int n = 0; n < 6; ++n) ld_row_together<G, M>(ra[n], CI + (int64_t)ia[n] * dpad, lane, ev);
#pragma unroll
            for (int n = 0; n < 6; ++n) ld_row_together<G, M>(rb[n], CU + (int64_t)ib[n] * dpad, lane, ev);
            cse_step_regs<G, M, MODE>(CI, ia, ra, wc, rab, s_sig, lane, ev, dpad);
            cse_step_regs<G, M, MODE>(CU, ib, rb, wu, rab, s_sig, lane, ev, dpad);
        } else {
            if (liveA) cse_step<G, M, MODE>(CI, ia, dA, wc, rab, s_sig, lane, ev, dpad);
            if (liveB) cse_step<G, M, MODE>(CU, ib, dB, wu, rab, s_sig, lane, ev, dpad);
        }
    }
    const int32_t* const dn = r + 12 * S;
    const float rr = alpha * 0.025f;
    if constexpr (RANK == 0) {
        // nemf: Opt_SGD on c (label +1), then on five negatives (label -1); WI rows move in place
        int32_t j[CSE_NEG];
        bool distinct = true;
#pragma unroll
        for (int n = 0; n < CSE_NEG; ++n) {
            j[n] = dn[n];
            distinct = distinct && j[n] != c;
#pragma unroll
            for (int k = 0; k < n; ++k) distinct = distinct && j[n] != j[k];
        }
        float wj[CSE_NEG][M];
        if (distinct) {
#pragma unroll
            for (int n = 0; n < CSE_NEG; ++n) ld_row_together<G, M>(wj[n], WI + (int64_t)j[n] * dpad, lane, ev);
        }
        float back[M];
        {
            const float a_ = alpha * (1.0f - cse_dot<G, M>(wu, wc));
#pragma unroll
            for (int m = 0; m < M; ++m) {
                back[m] = __builtin_fmaf(-rr, wu[m], __builtin_fmaf(a_, wc[m], 0.0f));
                wc[m] = __builtin_fmaf(a_, wu[m], __builtin_fmaf(-rr, wc[m], wc[m]));
            }
        }
#pragma unroll
        for (int n = 0; n < CSE_NEG; ++n) {
            float* const qj = WI + (int64_t)j[n] * dpad;
            const bool ejc = j[n] == c;
            if (!distinct) {
                if (ejc) {
#pragma unroll
                    for (int m = 0; m < M; ++m) wj[n][m] = wc[m];
                } else {
                    ld_row<G, M>(wj[n], qj, lane, ev);
                }
            }
            const float a_ = alpha * (-1.0f - cse_dot<G, M>(wu, wj[n]));
            float nj[M];
#pragma unroll
            for (int m = 0; m < M; ++m) {
                back[m] = __builtin_fmaf(-rr, wu[m], __builtin_fmaf(a_, wj[n][m], back[m]));
                nj[m] = __builtin_fmaf(a_, wu[m], __builtin_fmaf(-rr, wj[n][m], wj[n][m]));
            }
            if (ejc) {
#pragma unroll
                for (int m = 0; m < M; ++m) wc[m] = nj[m];
            } else {
                cse_put<G, M, MODE>(qj, nj, wj[n], lane, ev, dpad);
            }
        }
#pragma unroll
        for (int m = 0; m < M; ++m) wu[m] = wu[m] + back[m];
    } else {
        // nerank: the first negative with f < 1 updates, then the loop breaks; the gates
        // before it see untouched rows, so the rows come eight at a time
        constexpr int B = 8;
        bool done = false;
#pragma unroll 1
        for (int b0 = 0; b0 < CSE_RANK_NEG && !done; b0 += B) {
            int32_t j[B];
            float wj[B][M];
#pragma unroll
            for (int n = 0; n < B; ++n) {
                j[n] = dn[b0 + n];
                ld_row_together<G, M>(wj[n], WI + (int64_t)(j[n] < 0 ? 0 : j[n]) * dpad, lane, ev);
            }
#pragma unroll
            for (int n = 0; n < B; ++n) {
                if (j[n] < 0) done = true;   // the draws stopped here
                if (done) continue;
                const bool ejc = j[n] == c;
                float x[M], p = 0.0f;
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    if (ejc) wj[n][m] = wc[m];
                    x[m] = wc[m] - wj[n][m];
                    p = __builtin_fmaf(wu[m], x[m], p);
                }
                const float f = group_sum<G>(p);
                ++tested;
                if (!(f < 1.0f)) continue;
                done = true;
                ++updated;
                const float gg = fast_sigmoid(-f, s_sig) * alpha;
                float nj[M];
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    const float ve = gg * x[m], ce = gg * wu[m];
                    // the reference's per-element order on the shared location (j == c):
                    // decay c, decay j, decay v, c += ce, j -= ce, v += ve
                    float ac = wc[m], aj = wj[n][m];
                    ac = __builtin_fmaf(-rr, ac, ac);
                    if (ejc) aj = ac;
                    aj = __builtin_fmaf(-rr, aj, aj);
                    if (ejc) ac = aj;
                    wu[m] = __builtin_fmaf(-rr, wu[m], wu[m]);
                    ac = ac + ce;
                    if (ejc) aj = ac;
                    aj = aj - ce;
                    if (ejc) ac = aj;
                    wu[m] = wu[m] + ve;
                    wc[m] = ac;
                    nj[m] = aj;
                }
                if (!ejc) cse_put<G, M, MODE>(WI + (int64_t)j[n] * dpad, nj, wj[n], lane, ev, dpad);
            }
        }
    }
    cse_put<G, M, MODE>(qu, wu, u0, lane, ev, dpad);
    cse_put<G, M, MODE>(qc, wc, c0, lane, ev, dpad);
}

template <int G, int M, int MODE, int RANK>
__global__ void __launch_bounds__(256) cse_train_kernel(CseArgs a) {
    __shared__ float s_sig[1001];
    for (int k = threadIdx.x; k < 1001; k += blockDim.x) s_sig[k] = a.sig[k];
    __syncthreads();
    const uint64_t RW = (uint64_t)cse_width(a.steps, RANK);
    const int lane = threadIdx.x & (G - 1);
    const uint64_t gpb = blockDim.x / G, gib = threadIdx.x / G;
    const uint64_t count = a.count;
    bool ev[M];
    row_valid<G, M>(ev, lane, a.dpad);
    unsigned n_tested = 0, n_updated = 0;   // this group's, since the last counter add
    auto run = [&](uint64_t t) {
        cse_sample<G, M, MODE, RANK>(a, s_sig, lane, ev, a.rec + t * RW, alpha_at(a.begin + t, a.alpha0, a.total),
                                     n_tested, n_updated);
    };
    if (a.mode == SMORE_SERIAL) {
        // serial: one group, samples strictly in order
        if (blockIdx.x != 0 || gib != 0) return;
        unsigned long long tt = 0, tu = 0;
        for (uint64_t t = 0; t < count; ++t) {
            run(t);
            tt += n_tested;
            tu += n_updated;
            n_tested = n_updated = 0;
        }
        if (lane == 0 && RANK) {
            atomicAdd(a.stats, tt);
            atomicAdd(a.stats + 1, tu);
        }
        return;
    }
    // chunks of ch_rounds rounds handed out from a.work, as in warp_train_kernel
    __shared__ uint64_t s_next;
    uint64_t ch_rounds = count / ((uint64_t)gridDim.x * gpb * 16u);
    ch_rounds = ch_rounds < 8 ? 8 : ch_rounds > CH_ROUNDS ? CH_ROUNDS : ch_rounds;
    const uint64_t span = ch_rounds * gpb;
    for (;;) {
        __syncthreads();   // every wave has read the previous s_next
        if (threadIdx.x == 0) s_next = atomicAdd(a.work, 1ull) * span;
        __syncthreads();
        const uint64_t c0 = s_next;
        if (c0 >= count) break;
        const uint64_t lim = c0 + span < count ? c0 + span : count;
        for (uint64_t t = c0 + gib; t < lim; t += gpb) run(t);
        if constexpr (RANK != 0) {
            // the chunk's counts: one add per wave (a chunk is at most 128 rounds of 16 gates)
            uint32_t ct = lane == 0 ? n_tested : 0u, cu = lane == 0 ? n_updated : 0u;
            n_tested = n_updated = 0;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                ct += __shfl_xor(ct, m, 64);
                cu += __shfl_xor(cu, m, 64);
            }
            if ((threadIdx.x & 63) == 0 && ct) {
                atomicAdd(a.stats, (unsigned long long)ct);
                if (cu) atomicAdd(a.stats + 1, (unsigned long long)cu);
            }
        }
    }
}

// the (G, M) ladder; a unit (train_cse_<s|a>.hip) exports it as its update_symbol
// specialisations: KMAX = the direct term's negatives, 5 nemf, 16 nerank
template <int KMAX, int MODE>
const void* cse_symbol(int dpad, int) {
    static_assert(KMAX == CSE_NEG || KMAX == CSE_RANK_NEG, "nemf or nerank");
    const int G = lanes_of(dpad), M = regs_of(dpad);
#define X(g, m) \
    if (G == g && M == m) return (const void*)cse_train_kernel<g, m, MODE, (KMAX == CSE_RANK_NEG)>;
    SMORE_FOR_EACH_GM(X)
#undef X
    return nullptr;
}

}  // namespace smore

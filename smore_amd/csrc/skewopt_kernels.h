// skewopt_kernels.h -- the Skew-OPT update kernel for gfx950 (template).
//
// SPR::Train (src/model/SkewOPT.cpp:88-93) calls proNet::UpdateSBPRPair
// (src/proNet.cpp:1517-1566, Opt_SBPRSGD :1070-1098) on the ONE table: per
// sample one positive pair (v, i) and sixteen uniform negatives.  Per negative
// j: x = T[i] - T[j], f = T[v] . x, g = (f - xi) / omega; g > 2 skips it,
// g < -2 is clamped; p = g^eta, chain = p / g, gg = fastSigmoid(-p) chain /
// omega alpha; ve += gg x, ce = gg T[v], both rows decay by alpha 0.01 and move
// by +-ce.  After the sixteen, if any passed (up of them): T[v] decays and
// moves by ve / up.  All 18 ids come pre-drawn in the record (launch_draw with
// K = 16).  DESIGN.md 12c.
//
// One lane group of G lanes per sample (device_common.h row layout).  T[v],
// T[i] and ve stay in registers over the sixteen negatives.  When the 18 ids
// are pairwise distinct the negative rows are requested together (all sixteen,
// or two batches of eight for M = 8), T[i] is written once after the loop and
// every passed negative row once.  Otherwise the sample runs in the
// reference's memory order: a row that is v or i is taken from the registers
// that hold it, every other negative row is read after the previous
// negative's row was written.  The groups of a wave pass different gates:
// every cross-lane step is a group-width shuffle, no workgroup barrier inside
// a chunk.
#pragma once
#include "hoprec_kernels.h"

namespace smore {

// a / b as the fp32 rule takes every quotient (tests/c/skewopt_spec.c): the
// fp64 quotient of the two fp32 values, rounded once
__device__ __forceinline__ float skew_quot(float a, float b) { return (float)((double)a / (double)b); }

// the gate and the step size of one negative from its dot f; false: gated
__device__ __forceinline__ bool skew_gate(const SkewOptArgs& a, const float* s_sig, float f, float alpha, float& gg) {
    float g = skew_quot(f - a.xi, a.omega);
    if (g > 2.0f) return false;
    if (g < -2.0f) g = -2.0f;
    float p = 1.0f;
    for (int e = 0; e < a.eta; ++e) p = p * g;
    // g == 0 (f == xi): the limit of p / g, where the reference divides 0 by 0
    const float chain = g == 0.0f ? (a.eta >= 2 ? 0.0f : 1.0f) : skew_quot(p, g);
    gg = fast_sigmoid(-p, s_sig) * chain;
    gg = skew_quot(gg, a.omega);
    gg = gg * alpha;
    return true;
}

// One sample on record r = {v, i, j_0..j_15} (tagged ids) at learning rate
// alpha.  Returns the gates passed.
template <int G, int M, int MODE>
__device__ __forceinline__ unsigned skewopt_sample(const SkewOptArgs& a, const float* s_sig, int lane,
                                                   const bool (&ev)[M], const int32_t* r, float alpha) {
    constexpr int B = M > 4 ? 8 : SKEW_NEG;   // negative rows in flight together
    const int dpad = a.dpad;
    // the 18 ids in five 16-B words (the record is 32 words wide)
    int32_t id[20];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const i32x4 w = *reinterpret_cast<const i32x4*>(r + 4 * q);
#pragma unroll
        for (int k = 0; k < 4; ++k) id[4 * q + k] = w[k];
    }
    if (id[1] < 0) return 0;   // a source without out-edges (counted by the draw kernel)
    bool distinct = true;
#pragma unroll
    for (int k = 0; k < 2 + SKEW_NEG; ++k) {
        id[k] = untag(id[k]);
#pragma unroll
        for (int q = 0; q < k; ++q) distinct = distinct && id[k] != id[q];
    }
    const int32_t v = id[0], i = id[1];
    float* const qv = a.T + (int64_t)v * dpad;
    float* const qi = a.T + (int64_t)i * dpad;
    const float rd = alpha * 0.01f;
    const bool eiv = i == v;
    float wv[M], wi[M], v0[M], i0[M], ve[M];
    ld_row<G, M>(wv, qv, lane, ev);
    if (eiv) {
#pragma unroll
        for (int m = 0; m < M; ++m) wi[m] = wv[m];
    } else {
        ld_row<G, M>(wi, qi, lane, ev);
    }
#pragma unroll
    for (int m = 0; m < M; ++m) {
        v0[m] = wv[m];
        i0[m] = wi[m];
        ve[m] = 0.0f;
    }
    unsigned up = 0;
    if (distinct) {
#pragma unroll
        for (int b0 = 0; b0 < SKEW_NEG; b0 += B) {
            float wj[B][M];
#pragma unroll
            for (int n = 0; n < B; ++n) ld_row_together<G, M>(wj[n], a.T + (int64_t)id[2 + b0 + n] * dpad, lane, ev);
#pragma unroll
            for (int n = 0; n < B; ++n) {
                float x[M], p = 0.0f;
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    x[m] = wi[m] - wj[n][m];
                    p = __builtin_fmaf(wv[m], x[m], p);
                }
                float gg;
                if (!skew_gate(a, s_sig, group_sum<G>(p), alpha, gg)) continue;
                ++up;
                float nj[M];
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    ve[m] = __builtin_fmaf(gg, x[m], ve[m]);
                    const float ce = __builtin_fmaf(gg, wv[m], 0.0f);   // the reference adds to a zeroed vector
                    wi[m] = __builtin_fmaf(-rd, wi[m], wi[m]) + ce;
                    nj[m] = __builtin_fmaf(-rd, wj[n][m], wj[n][m]) - ce;
                }
                float* const qj = a.T + (int64_t)id[2 + b0 + n] * dpad;
                if constexpr (MODE == MODE_ATOMIC) {
#pragma unroll
                    for (int m = 0; m < M; ++m) nj[m] -= wj[n][m];
                    atomic_row<G, M>(qj, nj, lane, dpad);
                } else {
                    st_row<G, M>(qj, nj, lane, ev);
                }
            }
        }
    } else {
        // in the reference's memory order; the ids are read from the record again
        // (a register array indexed by the loop counter would live in scratch)
#pragma unroll 1
        for (int n = 0; n < SKEW_NEG; ++n) {
            const int32_t j = untag(r[2 + n]);
            float* const qj = a.T + (int64_t)j * dpad;
            const bool ejv = j == v, eij = j == i;
            float wj[M];
            if (ejv) {
#pragma unroll
                for (int m = 0; m < M; ++m) wj[m] = wv[m];
            } else if (eij) {
#pragma unroll
                for (int m = 0; m < M; ++m) wj[m] = wi[m];
            } else {
                ld_row<G, M>(wj, qj, lane, ev);
            }
            float x[M], p = 0.0f;
#pragma unroll
            for (int m = 0; m < M; ++m) {
                x[m] = wi[m] - wj[m];
                p = __builtin_fmaf(wv[m], x[m], p);
            }
            float gg;
            if (!skew_gate(a, s_sig, group_sum<G>(p), alpha, gg)) continue;
            ++up;
            float nj[M];
#pragma unroll
            for (int m = 0; m < M; ++m) {
                ve[m] = __builtin_fmaf(gg, x[m], ve[m]);
                const float ce = __builtin_fmaf(gg, wv[m], 0.0f);
                // the reference's per-element order on the shared location:
                // decay i, decay j, i += ce, j -= ce
                float ai = wi[m], aj = wj[m];
                ai = __builtin_fmaf(-rd, ai, ai);
                if (eij) aj = ai;
                aj = __builtin_fmaf(-rd, aj, aj);
                if (eij) ai = aj;
                ai = ai + ce;
                if (eij) aj = ai;
                aj = aj - ce;
                if (eij) ai = aj;
                wi[m] = ai;
                nj[m] = aj;
            }
            // rows that are v keep living in wv (i == v: wi is T[v]; j == v: so is the new j row)
            if (eiv) {
#pragma unroll
                for (int m = 0; m < M; ++m) wv[m] = wi[m];
            }
            if (ejv) {
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    wv[m] = nj[m];
                    if (eiv) wi[m] = nj[m];
                }
            }
            if (!ejv && !eij) {
                if constexpr (MODE == MODE_ATOMIC) {
#pragma unroll
                    for (int m = 0; m < M; ++m) nj[m] -= wj[m];
                    atomic_row<G, M>(qj, nj, lane, dpad);
                } else {
                    st_row<G, M>(qj, nj, lane, ev);
                }
            }
        }
    }
    if (up == 0) return 0;
    // T[v]; i == v: the row wi holds too
    const float upf = (float)up;
#pragma unroll
    for (int m = 0; m < M; ++m) wv[m] = __builtin_fmaf(-rd, wv[m], wv[m]) + skew_quot(ve[m], upf);
    if constexpr (MODE == MODE_ATOMIC) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            v0[m] = wv[m] - v0[m];
            i0[m] = wi[m] - i0[m];
        }
        if (!eiv) atomic_row<G, M>(qi, i0, lane, dpad);
        atomic_row<G, M>(qv, v0, lane, dpad);
    } else {
        if (!eiv) st_row<G, M>(qi, wi, lane, ev);
        st_row<G, M>(qv, wv, lane, ev);
    }
    return up;
}

template <int G, int M, int MODE>
__global__ void __launch_bounds__(256) skewopt_train_kernel(SkewOptArgs a) {
    __shared__ float s_sig[1001];
    for (int k = threadIdx.x; k < 1001; k += blockDim.x) s_sig[k] = a.sig[k];
    __syncthreads();
    constexpr uint64_t RW = rec_width(SKEWOPT_KMAX);
    const int lane = threadIdx.x & (G - 1);
    const uint64_t gpb = blockDim.x / G, gib = threadIdx.x / G;
    const uint64_t count = a.count;
    bool ev[M];
    row_valid<G, M>(ev, lane, a.dpad);
    unsigned n_passed = 0, n_upd = 0;   // this group's, since the last counter add
    auto run = [&](uint64_t t) {
        const unsigned up = skewopt_sample<G, M, MODE>(a, s_sig, lane, ev, a.rec + t * RW,
                                                      alpha_at(a.begin + t, a.alpha0, a.total));
        n_passed += up;
        n_upd += up ? 1u : 0u;
    };
    if (a.mode == SMORE_SERIAL) {
        // serial: one group, samples strictly in order
        if (blockIdx.x != 0 || gib != 0) return;
        unsigned long long tp = 0, tu = 0;
        for (uint64_t t = 0; t < count; ++t) {
            run(t);
            tp += n_passed;
            tu += n_upd;
            n_passed = n_upd = 0;
        }
        if (lane == 0) {
            atomicAdd(a.stats, tp);
            atomicAdd(a.stats + 1, tu);
        }
        return;
    }
    // chunks of ch_rounds rounds handed out from a.work, as in hoprec_train_kernel
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
        // the chunk's counts: one add per wave (a chunk is at most 128 rounds of 16 gates)
        uint32_t cp = lane == 0 ? n_passed : 0u, cu = lane == 0 ? n_upd : 0u;
        n_passed = n_upd = 0;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            cp += __shfl_xor(cp, m, 64);
            cu += __shfl_xor(cu, m, 64);
        }
        if ((threadIdx.x & 63) == 0 && cp) {
            atomicAdd(a.stats, (unsigned long long)cp);
            atomicAdd(a.stats + 1, (unsigned long long)cu);
        }
    }
}

// the (G, M) ladder; a unit (train_skewopt_<s|a>.hip) exports it as its
// update_symbol specialisation (train_kernels.h SMORE_UPDATE_INST)
template <int KMAX, int MODE>
const void* skewopt_symbol(int dpad, int) {
    static_assert(KMAX == SKEWOPT_KMAX, "one bucket");
    const int G = lanes_of(dpad), M = regs_of(dpad);
#define X(g, m) \
    if (G == g && M == m) return (const void*)skewopt_train_kernel<g, m, MODE>;
    SMORE_FOR_EACH_GM(X)
#undef X
    return nullptr;
}

}  // namespace smore

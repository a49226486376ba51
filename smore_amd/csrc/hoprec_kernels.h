// hoprec_kernels.h -- the HOP-REC update kernel for gfx950 (template).
//
// HBPR::Train (src/model/HBPR.cpp:94-114) calls proNet::UpdateFBPRPair
// (src/proNet.cpp:1458-1515, Opt_FBPRSGD :1014-1031) walk_steps times per
// sample on the ONE table: step w runs at rate alpha / w and margin 1 / w on
// {v, i_w, j_w0..j_w4}.  Per negative n: x = T[i] - T[j], f = T[v] . x; the
// gate f > margin skips it, otherwise g = fastSigmoid(-f) rate, ve += g x,
// ce = g T[v], both rows decay by rate 0.0025 and move by +-ce.  After the
// five, if any passed (up of them): T[v] decays by rate 0.025 and moves by
// ve / up.  Every id comes pre-drawn in the record (train_hoprec_draw.hip):
// unlike WARP nothing but the gate depends on the tables, so a step's five
// negative rows are requested together.  DESIGN.md 12b.
//
// One lane group of G lanes per sample (device_common.h row layout).  T[v]
// stays in registers over the sample's steps, T[i_w] over its step.  When two
// of a step's seven ids coincide the step runs in order instead: a row that
// is v or i_w is taken from the registers that hold it, every other negative
// row is read after the previous negative's row was written, so same-id rows
// see each other's result before the next operation as the reference's
// vector<double> rows do.  The groups of a wave pass different gates: every
// cross-lane step is a group-width shuffle, no workgroup barrier inside a chunk.
#pragma once
#include "train_kernels.h"

namespace smore {

// alpha / w and 1 / w as the fp32 rule takes them (tests/c/hoprec_spec.c):
// the fp64 quotient, rounded once
__device__ __forceinline__ float hoprec_rate(float alpha, int w) { return (float)((double)alpha / (double)w); }
__device__ __forceinline__ float hoprec_margin(int w) { return (float)(1.0 / (double)w); }

// r = row without a branch: a chunk that does not exist reads the row's first
// chunk (always there, dpad >= 4) and is zeroed by a select, so consecutive
// calls put their loads in flight back to back -- ld_row's per-chunk `if`
// makes the compiler wait for each load before the next is issued
template <int G, int M>
__device__ __forceinline__ void ld_row_together(float (&r)[M], const float* row, int lane, const bool (&ev)[M]) {
#pragma unroll
    for (int k = 0; k < M / 4; ++k) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(row + (ev[4 * k] ? 4 * (lane + G * k) : 0));
#pragma unroll
        for (int i = 0; i < 4; ++i) r[4 * k + i] = ev[4 * k] ? x[i] : 0.0f;
    }
}

// One sample: record r (hoprec_width(a.steps) words) at learning rate alpha.
// tested / passed: the gates this sample evaluated / that let an update through.
template <int G, int M, int MODE>
__device__ __forceinline__ void hoprec_sample(const HopRecArgs& a, const float* s_sig, int lane, const bool (&ev)[M],
                                              const int32_t* r, float alpha, unsigned& tested, unsigned& passed) {
    const int dpad = a.dpad;
    const int32_t tv = r[0];
    if (tv < 0 || r[1] < 0) return;
    const int32_t v = untag(tv);
    float* const qv = a.T + (int64_t)v * dpad;
    float wv[M], v0[M];
    ld_row<G, M>(wv, qv, lane, ev);
#pragma unroll
    for (int m = 0; m < M; ++m) v0[m] = wv[m];
    bool v_dirty = false;
    for (int w = 1; w <= a.steps; ++w) {
        const int32_t* const o = r + 1 + (1 + HOPREC_NEG) * (w - 1);
        // the step's six words in one round trip (all inside the record, whatever they hold)
        int32_t ow[1 + HOPREC_NEG];
#pragma unroll
        for (int n = 0; n <= HOPREC_NEG; ++n) ow[n] = o[n];
        if (ow[0] < 0) break;
        const int32_t i = untag(ow[0]);
        int32_t j[HOPREC_NEG];
#pragma unroll
        for (int n = 0; n < HOPREC_NEG; ++n) j[n] = untag(ow[1 + n]);
        bool distinct = i != v;
#pragma unroll
        for (int n = 0; n < HOPREC_NEG; ++n) {
            distinct = distinct && j[n] != v && j[n] != i;
#pragma unroll
            for (int k = 0; k < n; ++k) distinct = distinct && j[n] != j[k];
        }
        const float rate = hoprec_rate(alpha, w), margin = hoprec_margin(w);
        const float rd = rate * 0.0025f, rdv = rate * 0.025f;
        float* const qi = a.T + (int64_t)i * dpad;
        const bool eiv = i == v;
        float wi[M], i0[M], ve[M], wj[HOPREC_NEG][M];
        if (distinct) {
            // T[i_w] and the step's five negative rows in flight together
            ld_row_together<G, M>(wi, qi, lane, ev);
#pragma unroll
            for (int n = 0; n < HOPREC_NEG; ++n) ld_row_together<G, M>(wj[n], a.T + (int64_t)j[n] * dpad, lane, ev);
        } else if (eiv) {
#pragma unroll
            for (int m = 0; m < M; ++m) wi[m] = wv[m];
        } else {
            ld_row<G, M>(wi, qi, lane, ev);
        }
#pragma unroll
        for (int m = 0; m < M; ++m) {
            i0[m] = wi[m];
            ve[m] = 0.0f;
        }
        unsigned up = 0;
#pragma unroll
        for (int n = 0; n < HOPREC_NEG; ++n) {
            float* const qj = a.T + (int64_t)j[n] * dpad;
            const bool ejv = j[n] == v, eij = j[n] == i;
            if (!distinct) {
                if (ejv) {
#pragma unroll
                    for (int m = 0; m < M; ++m) wj[n][m] = wv[m];
                } else if (eij) {
#pragma unroll
                    for (int m = 0; m < M; ++m) wj[n][m] = wi[m];
                } else {
                    ld_row<G, M>(wj[n], qj, lane, ev);
                }
            }
            float x[M], p = 0.0f;
#pragma unroll
            for (int m = 0; m < M; ++m) {
                x[m] = wi[m] - wj[n][m];
                p = __builtin_fmaf(wv[m], x[m], p);
            }
            const float f = group_sum<G>(p);
            ++tested;
            if (f > margin) continue;
            ++up;
            const float gg = fast_sigmoid(-f, s_sig) * rate;
            float nj[M];
#pragma unroll
            for (int m = 0; m < M; ++m) {
                ve[m] = __builtin_fmaf(gg, x[m], ve[m]);
                const float ce = __builtin_fmaf(gg, wv[m], 0.0f);   // the reference adds to a zeroed vector
                // the reference's per-element order on the shared location:
                // decay i, decay j, i += ce, j -= ce
                float ai = wi[m], aj = wj[n][m];
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
                v_dirty = true;
            }
            if (ejv) {
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    wv[m] = nj[m];
                    if (eiv) wi[m] = nj[m];
                }
                v_dirty = true;
            }
            if (!ejv && !eij) {
                if constexpr (MODE == MODE_ATOMIC) {
#pragma unroll
                    for (int m = 0; m < M; ++m) nj[m] -= wj[n][m];
                    atomic_row<G, M>(qj, nj, lane, dpad);
                } else {
                    st_row<G, M>(qj, nj, lane, ev);
                }
            }
        }
        passed += up;
        if (up == 0) continue;
        // T[v] of this step; i == v: the row wi holds
        const float upf = (float)up;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            float av = wv[m];
            av = __builtin_fmaf(-rdv, av, av);
            av = av + (float)((double)ve[m] / (double)upf);
            wv[m] = av;
        }
        v_dirty = true;
        if (!eiv) {
            // the step's rows are in memory before the next step gathers
            if constexpr (MODE == MODE_ATOMIC) {
#pragma unroll
                for (int m = 0; m < M; ++m) i0[m] = wi[m] - i0[m];
                atomic_row<G, M>(qi, i0, lane, dpad);
            } else {
                st_row<G, M>(qi, wi, lane, ev);
            }
        }
    }
    if (!v_dirty) return;
    if constexpr (MODE == MODE_ATOMIC) {
#pragma unroll
        for (int m = 0; m < M; ++m) v0[m] = wv[m] - v0[m];
        atomic_row<G, M>(qv, v0, lane, dpad);
    } else {
        st_row<G, M>(qv, wv, lane, ev);
    }
}

template <int G, int M, int MODE>
__global__ void __launch_bounds__(256) hoprec_train_kernel(HopRecArgs a) {
    __shared__ float s_sig[1001];
    for (int k = threadIdx.x; k < 1001; k += blockDim.x) s_sig[k] = a.sig[k];
    __syncthreads();
    const uint64_t RW = (uint64_t)hoprec_width(a.steps);
    const int lane = threadIdx.x & (G - 1);
    const uint64_t gpb = blockDim.x / G, gib = threadIdx.x / G;
    const uint64_t count = a.count;
    bool ev[M];
    row_valid<G, M>(ev, lane, a.dpad);
    unsigned n_tested = 0, n_passed = 0;   // this group's, since the last counter add
    auto run = [&](uint64_t t) {
        hoprec_sample<G, M, MODE>(a, s_sig, lane, ev, a.rec + t * RW, alpha_at(a.begin + t, a.alpha0, a.total), n_tested,
                                  n_passed);
    };
    if (a.mode == SMORE_SERIAL) {
        // serial: one group, samples strictly in order
        if (blockIdx.x != 0 || gib != 0) return;
        unsigned long long tt = 0, tp = 0;
        for (uint64_t t = 0; t < count; ++t) {
            run(t);
            tt += n_tested;
            tp += n_passed;
            n_tested = n_passed = 0;
        }
        if (lane == 0) {
            atomicAdd(a.stats, tt);
            atomicAdd(a.stats + 1, tp);
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
        // the chunk's counts: one add per wave (a chunk is at most 128 rounds of 50 gates)
        uint32_t ct = lane == 0 ? n_tested : 0u, cp = lane == 0 ? n_passed : 0u;
        n_tested = n_passed = 0;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            ct += __shfl_xor(ct, m, 64);
            cp += __shfl_xor(cp, m, 64);
        }
        if ((threadIdx.x & 63) == 0 && ct) {
            atomicAdd(a.stats, (unsigned long long)ct);
            if (cp) atomicAdd(a.stats + 1, (unsigned long long)cp);
        }
    }
}

// the (G, M) ladder; a unit (train_hoprec_<s|a>.hip) exports it as its
// update_symbol specialisation (train_kernels.h SMORE_UPDATE_INST)
template <int KMAX, int MODE>
const void* hoprec_symbol(int dpad, int) {
    static_assert(KMAX == HOPREC_KMAX, "one bucket");
    const int G = lanes_of(dpad), M = regs_of(dpad);
#define X(g, m) \
    if (G == g && M == m) return (const void*)hoprec_train_kernel<g, m, MODE>;
    SMORE_FOR_EACH_GM(X)
#undef X
    return nullptr;
}

}  // namespace smore

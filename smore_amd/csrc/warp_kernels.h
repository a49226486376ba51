// warp_kernels.h -- the WARP update kernel for gfx950 (template).
//
// proNet::UpdateWARPPair (src/proNet.cpp:1353-1403) as WARP::Train calls it
// (src/model/WARP.cpp:85-91): one table, negatives drawn ONE AT A TIME until
// one violates the margin (f < 1), at most 32, and only then one update of the
// three rows v, i, j.  Unlike every other rule here the number of draws a
// sample uses depends on the tables, so the negatives of trials 1..31 are
// drawn in this kernel (trial 0's comes pre-drawn in the record, with v and i:
// launch_draw with K = 1).  DESIGN.md "WARP".
//
// One lane group of G lanes per sample (device_common.h row layout).  The
// groups of a wave leave the trial loop at different trials: every cross-lane
// step inside it is a group-width shuffle, and there is no workgroup barrier
// between a chunk's first and last sample.
#pragma once
#include "train_kernels.h"

namespace smore {

// speculative prefetch of trial n+1's negative row while trial n is reduced
// (the later trials' ids do not depend on the tables); a build-time choice,
// measured in DESIGN.md "WARP"
#ifndef SMORE_WARP_SPEC
#define SMORE_WARP_SPEC 0
#endif

// the negative of trial n >= 1 of sample s: slots 4 + 2n (index), 5 + 2n (p)
// of unit s, stream 0 -- block 1 + n/2, components 2(n&1), 2(n&1) + 1
__device__ __forceinline__ int32_t warp_negative(const DevGraph& g, uint64_t seed, uint64_t s, int n) {
    const uint4 b = philox_block(seed, 0, s, 1u + (uint32_t)(n >> 1));
    return untag((n & 1) ? negative_sample(g, b.z, b.w) : negative_sample(g, b.x, b.y));
}

// One sample on rows v, i and the trial negatives (untagged ids).  Returns the
// trials executed; hit = one of them had f < 1 and the rows were updated.
// Aliasing (two of v, i, j equal) follows the reference's per-element order on
// the shared memory location: decay i, decay j, decay v, i += ce, j -= ce,
// v += ve, each result seen by the aliases before the next step.
template <int G, int M, int MODE>
__device__ __forceinline__ int warp_sample(const WarpArgs& a, const float* s_sig, int lane, const bool (&ev)[M],
                                           uint64_t s, int32_t v, int32_t i, int32_t j, float alpha, bool& hit) {
    const int dpad = a.dpad;
    float wv[M], wi[M], wj[M], x[M];
    ld_row<G, M>(wv, a.T + (int64_t)v * dpad, lane, ev);
    ld_row<G, M>(wi, a.T + (int64_t)i * dpad, lane, ev);
    ld_row<G, M>(wj, a.T + (int64_t)j * dpad, lane, ev);
#if SMORE_WARP_SPEC
    float wn[M];
    int32_t jn = warp_negative(a.g, a.seed, s, 1);
    ld_row<G, M>(wn, a.T + (int64_t)jn * dpad, lane, ev);
#endif
    float f = 0.0f;
    int n = 0;
    hit = false;
    for (;;) {
        float p = 0.0f;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            x[m] = wi[m] - wj[m];
            p = __builtin_fmaf(wv[m], x[m], p);
        }
        f = group_sum<G>(p);
        ++n;
        if (f < 1.0f) {
            hit = true;
            break;
        }
        if (n == WARP_TRIALS) break;
#if SMORE_WARP_SPEC
        j = jn;
#pragma unroll
        for (int m = 0; m < M; ++m) wj[m] = wn[m];
        if (n + 1 < WARP_TRIALS) {
            jn = warp_negative(a.g, a.seed, s, n + 1);
            ld_row<G, M>(wn, a.T + (int64_t)jn * dpad, lane, ev);
        }
#else
        j = warp_negative(a.g, a.seed, s, n);
        ld_row<G, M>(wj, a.T + (int64_t)j * dpad, lane, ev);
#endif
    }
    if (!hit) return n;
    const float gg = fast_sigmoid(-f, s_sig) * alpha;
    const float r = alpha * 0.0025f;
    const bool eij = i == j, eiv = i == v, ejv = j == v;
    float ni[M], nj[M], nv[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const float ce = __builtin_fmaf(gg, wv[m], 0.0f);   // the reference adds to a zeroed vector
        const float ve = __builtin_fmaf(gg, x[m], 0.0f);
        float ai = wi[m], aj = wj[m], av = wv[m];
        ai = __builtin_fmaf(-r, ai, ai);
        if (eij) aj = ai;
        if (eiv) av = ai;
        aj = __builtin_fmaf(-r, aj, aj);
        if (eij) ai = aj;
        if (ejv) av = aj;
        av = __builtin_fmaf(-r, av, av);
        if (eiv) ai = av;
        if (ejv) aj = av;
        ai = ai + ce;
        if (eij) aj = ai;
        if (eiv) av = ai;
        aj = aj - ce;
        if (eij) ai = aj;
        if (ejv) av = aj;
        av = av + ve;
        if (eiv) ai = av;
        if (ejv) aj = av;
        ni[m] = ai;
        nj[m] = aj;
        nv[m] = av;
    }
    // scatter: every distinct row once (aliased rows hold the same final value)
    float* const qi = a.T + (int64_t)i * dpad;
    float* const qj = a.T + (int64_t)j * dpad;
    float* const qv = a.T + (int64_t)v * dpad;
    if constexpr (MODE == WARP_ATOMIC) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            ni[m] -= wi[m];
            nj[m] -= wj[m];
            nv[m] -= wv[m];
        }
        atomic_row<G, M>(qi, ni, lane, dpad);
        if (!eij) atomic_row<G, M>(qj, nj, lane, dpad);
        if (!eiv && !ejv) atomic_row<G, M>(qv, nv, lane, dpad);
    } else {
        st_row<G, M>(qi, ni, lane, ev);
        if (!eij) st_row<G, M>(qj, nj, lane, ev);
        if (!eiv && !ejv) st_row<G, M>(qv, nv, lane, ev);
    }
    return n;
}

template <int G, int M, int MODE>
__global__ void __launch_bounds__(256) warp_train_kernel(WarpArgs a) {
    __shared__ float s_sig[1001];
    for (int k = threadIdx.x; k < 1001; k += blockDim.x) s_sig[k] = a.sig[k];
    __syncthreads();
    constexpr int RW = rec_width(WARP_KMAX);
    const int lane = threadIdx.x & (G - 1);
    const uint64_t gpb = blockDim.x / G, gib = threadIdx.x / G;
    const uint64_t count = a.count;
    bool ev[M];
    row_valid<G, M>(ev, lane, a.dpad);
    unsigned long long n_trials = 0, n_upd = 0;   // this group's, since the last counter add
    // record t: sample begin + t; i < 0: a source without out-edges (counted by the draw kernel)
    auto run = [&](const i32x4& r, uint64_t t) {
        if (r[1] < 0) return;
        bool hit;
        const uint64_t s = a.begin + t;
        n_trials += (unsigned long long)warp_sample<G, M, MODE>(a, s_sig, lane, ev, s, untag(r[0]), untag(r[1]), untag(r[2]),
                                                     alpha_at(s, a.alpha0, a.total), hit);
        n_upd += hit ? 1ull : 0ull;
    };
    if (a.mode == 2) {
        // serial: one group, samples strictly in order
        if (blockIdx.x != 0 || gib != 0) return;
        for (uint64_t t = 0; t < count; ++t) run(*reinterpret_cast<const i32x4*>(a.rec + t * RW), t);
        if (lane == 0) {
            atomicAdd(a.stats, n_trials);
            atomicAdd(a.stats + 1, n_upd);
        }
        return;
    }
    // Hogwild modes: chunks of ch_rounds rounds handed out from a.work, as in
    // edge_train_kernel; inside a chunk a group runs its samples on its own
    // Only the first a.groups groups of a block take samples (the plain-store
    // concurrency cap of train_warp.cpp); the others only keep the barriers.
    __shared__ uint64_t s_next;
    const uint64_t act = (uint64_t)a.groups < gpb ? (uint64_t)a.groups : gpb;
    uint64_t ch_rounds = count / ((uint64_t)gridDim.x * act * 16u);
    ch_rounds = ch_rounds < 8 ? 8 : ch_rounds > CH_ROUNDS ? CH_ROUNDS : ch_rounds;
    const uint64_t span = ch_rounds * act;
    for (;;) {
        __syncthreads();   // every wave has read the previous s_next
        if (threadIdx.x == 0) s_next = atomicAdd(a.work, 1ull) * span;
        __syncthreads();
        const uint64_t c0 = s_next;
        if (c0 >= count) break;
        const uint64_t lim = c0 + span < count ? c0 + span : count;
        uint64_t t = gib < act ? c0 + gib : lim;
        i32x4 r = {-1, -1, -1, -1};
        if (t < lim) r = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(a.rec + t * RW));
        for (; t < lim; t += act) {
            const i32x4 cur = r;
            if (t + act < lim) r = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(a.rec + (t + act) * RW));
            run(cur, t);
        }
        // the chunk's counts: one add per wave
        uint32_t ct = lane == 0 ? (uint32_t)n_trials : 0u, cu = lane == 0 ? (uint32_t)n_upd : 0u;
        n_trials = n_upd = 0;
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

// the (G, M) ladder; a unit (train_warp_<s|a>.hip) exports it as its
// update_symbol specialisation (train_kernels.h SMORE_UPDATE_INST)
template <int KMAX, int MODE>
const void* warp_symbol(int dpad, int) {
    static_assert(KMAX == WARP_KMAX, "one record width");
    const int G = lanes_of(dpad), M = regs_of(dpad);
#define X(g, m) \
    if (G == g && M == m) return (const void*)warp_train_kernel<g, m, MODE>;
    SMORE_FOR_EACH_GM(X)
#undef X
    return nullptr;
}

}  // namespace smore

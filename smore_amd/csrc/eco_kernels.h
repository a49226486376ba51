// eco_kernels.h -- the sampled-softmax choice (ECO) update kernel for gfx950 (template),
// on table 0 (w_vertex).
//
// proNet::UpdateDChoice (src/proNet.cpp:2221-2341) runs per sample, around one vertex v,
// five lists {c1, c2, n_0..n_{K-1}} of rows of the same table:
//   e1 = exp(W[v].W[c1]), e2 = exp(W[v].W[c2]), e_k = exp(W[v].W[n_k]), sum = sum_k e_k + e1 + e2
//   dev = W[c1] e1 + W[c2] e2 + sum_k W[n_k] e_k
//   back_v += alpha ((2 W[c1] e1 + W[c2] e2) / (2 e1 + e2) - dev / sum - reg W[v])
//   W[c1] += alpha (2 W[v] e1 / (2 e1 + e2) - W[v] e1 / sum - reg W[c1])
//   W[c2] += alpha (  W[v] e2 / (2 e1 + e2) - W[v] e2 / sum - reg W[c2])
//   W[n_k] -= alpha (W[v] e_k / sum + reg W[n_k]), k in order
// and W[v] += back_v after the fifth list.  Every id comes pre-drawn in the record
// {v, 5 x {c1, c2, n_0..n_{K-1}}} (train_eco_draw.hip), with the sample's clean flag.
// The arithmetic (exp32.h, one reciprocal per denominator, the fmaf order) is
// listed in DESIGN.md 12f and mirrored by tests/c/eco_spec.c eco_spec_f32.
//
// One lane group of G lanes per sample (device_common.h row layout).  W[v],
// back_v and dev live for the whole sample, a list's K + 2 scores for the list,
// in registers indexed at compile time (KMAX = the K bucket 5 / 10 / 20).  A
// list's c1 and c2 rows and its negative rows, the latter in batches of
// ECO_BATCH, are gathered into one of two register buffers; with K > ECO_BATCH
// the batches are gathered a second time (from L2) when their rows move.
//   clean sample (all ids pairwise distinct): no row is written before it is
//     read, so W[v] is read once, a list's rows are requested together and the
//     next list's c1, c2 and first batch are requested before this list's rows
//     are written; a row moves by the delta computed from its gathered value.
//   other samples run in the reference's memory order: a list's loads are issued
//     after every earlier write of the sample has completed; when v and the
//     list's ids are pairwise distinct its rows move by their gathered values,
//     otherwise every row that moves -- c1, then c2, then the negatives in
//     order -- is read again, with W[v], after the write before it has completed.
// A write is row += delta: one atomic add of the delta (atomic scatter) or a
// store of row + delta (plain stores, the serial mode).
#pragma once
#include "exp32.h"
#include "hoprec_kernels.h"

namespace smore {

template <int G, int M>
__device__ __forceinline__ float eco_dot(const float (&a)[M], const float (&b)[M]) {
    float p = 0.0f;
#pragma unroll
    for (int m = 0; m < M; ++m) p = __builtin_fmaf(a[m], b[m], p);
    return group_sum<G>(p);
}

// every vector-memory operation of this wave so far (loads, stores, atomic adds) has completed
__device__ __forceinline__ void eco_wait_memory() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// a list's rows in registers: c1, c2 and one batch of negatives
template <int M>
struct EcoBuf {
    float p[2][M];
    float n[ECO_BATCH][M];
};

// row q (holding `row`) += alpha (cf wv - reg row)
template <int G, int M, int MODE>
__device__ __forceinline__ void eco_move(float* q, const float (&row)[M], const float (&wv)[M], float cf, float alpha,
                                         float reg, int lane, const bool (&ev)[M], int dpad) {
    float dl[M];
#pragma unroll
    for (int m = 0; m < M; ++m) dl[m] = alpha * __builtin_fmaf(-reg, row[m], cf * wv[m]);
    if constexpr (MODE == MODE_ATOMIC) {
        atomic_row<G, M>(q, dl, lane, dpad);
    } else {
#pragma unroll
        for (int m = 0; m < M; ++m) dl[m] = row[m] + dl[m];
        st_row<G, M>(q, dl, lane, ev);
    }
}

// negatives k0 .. k0 + ECO_BATCH - 1 of the list `set` requested together (from K on: the
// list's c1 row again, never used)
template <int G, int M>
__device__ __forceinline__ void eco_gather(float (&n)[ECO_BATCH][M], const float* T, const int32_t* set, int k0, int K,
                                           int lane, const bool (&ev)[M], int dpad) {
#pragma unroll
    for (int b = 0; b < ECO_BATCH; ++b) {
        const int k = k0 + b;
        const int32_t id = set[k < K ? 2 + k : 0];
        ld_row_together<G, M>(n[b], T + (int64_t)id * dpad, lane, ev);
    }
}

// One sample: record r (eco_width(a.K) words) at learning rate alpha.
template <int G, int M, int MODE, int KMAX>
__device__ __forceinline__ void eco_sample(const EcoArgs& a, int lane, const bool (&ev)[M], const int32_t* r,
                                           unsigned flags, float alpha) {
    const bool clean = flags & 1u;
    constexpr int B = ECO_BATCH, NB = KMAX / B;
    const int dpad = a.dpad, K = a.K;
    const float reg = a.reg;
    float* const T = a.T;
    float* const qv = T + (int64_t)r[0] * dpad;
    float wv[M], back[M], dev[M];
    float e[KMAX];
#pragma unroll
    for (int m = 0; m < M; ++m) back[m] = 0.0f;
    EcoBuf<M> bufA, bufB;
    // c1, c2 and the first batch of list `set`
    auto request = [&](EcoBuf<M>& X, const int32_t* set) __attribute__((always_inline)) {
        ld_row_together<G, M>(X.p[0], T + (int64_t)set[0] * dpad, lane, ev);
        ld_row_together<G, M>(X.p[1], T + (int64_t)set[1] * dpad, lane, ev);
        eco_gather<G, M>(X.n, T, set, 0, K, lane, ev, dpad);
    };
    // list l: its rows are in X (clean) or requested here; Y takes the next list's
    auto list = [&](EcoBuf<M>& X, EcoBuf<M>& Y, int l) __attribute__((always_inline)) {
        const int32_t* const set = r + 1 + l * (2 + K);
        if (!clean) {
            eco_wait_memory();
            ld_row_together<G, M>(wv, qv, lane, ev);
            request(X, set);
        }
        const float e1 = exp32(eco_dot<G, M>(wv, X.p[0])), e2 = exp32(eco_dot<G, M>(wv, X.p[1]));
#pragma unroll
        for (int m = 0; m < M; ++m) dev[m] = __builtin_fmaf(X.p[1][m], e2, X.p[0][m] * e1);
        float sum = 0.0f;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            if (nb * B < K) {
                if (nb > 0) eco_gather<G, M>(X.n, T, set, nb * B, K, lane, ev, dpad);
#pragma unroll
                for (int b = 0; b < B; ++b) {
                    const float ek = nb * B + b < K ? exp32(eco_dot<G, M>(wv, X.n[b])) : 0.0f;
                    e[nb * B + b] = ek;
                    if (nb * B + b < K) {
                        sum = sum + ek;
#pragma unroll
                        for (int m = 0; m < M; ++m) dev[m] = __builtin_fmaf(X.n[b][m], ek, dev[m]);
                    }
                }
            }
        }
        sum = sum + e1;
        sum = sum + e2;
        const float is = 1.0f / sum, e11 = e1 + e1, id = 1.0f / (e11 + e2);
        const float g1 = e11 * id, g2 = e2 * id;
        const float cf1 = g1 - e1 * is, cf2 = g2 - e2 * is;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const float t = __builtin_fmaf(-is, dev[m], __builtin_fmaf(g1, X.p[0][m], g2 * X.p[1][m]));
            back[m] = __builtin_fmaf(alpha, __builtin_fmaf(-reg, wv[m], t), back[m]);
        }
        if ((flags >> (1 + l)) & 1u) {
            // v and the list's ids are pairwise distinct: no row of the list is written before it is read
            if (clean && l + 1 < ECO_LISTS) request(Y, set + (2 + K));
            eco_move<G, M, MODE>(T + (int64_t)set[0] * dpad, X.p[0], wv, cf1, alpha, reg, lane, ev, dpad);
            eco_move<G, M, MODE>(T + (int64_t)set[1] * dpad, X.p[1], wv, cf2, alpha, reg, lane, ev, dpad);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                if (nb * B < K) {
                    if (NB > 1 && K > B) eco_gather<G, M>(X.n, T, set, nb * B, K, lane, ev, dpad);
#pragma unroll
                    for (int b = 0; b < B; ++b)
                        if (nb * B + b < K)
                            eco_move<G, M, MODE>(T + (int64_t)set[2 + nb * B + b] * dpad, X.n[b], wv,
                                                 -(e[nb * B + b] * is), alpha, reg, lane, ev, dpad);
                }
            }
        } else {
            // the reference's memory order: each row that moves is read again, with W[v], after
            // the write before it
            auto again = [&](int32_t id, float cf) __attribute__((always_inline)) {
                float* const q = T + (int64_t)id * dpad;
                eco_wait_memory();
                ld_row_together<G, M>(X.p[0], qv, lane, ev);
                ld_row_together<G, M>(X.p[1], q, lane, ev);
                eco_move<G, M, MODE>(q, X.p[1], X.p[0], cf, alpha, reg, lane, ev, dpad);
            };
            again(set[0], cf1);
            again(set[1], cf2);
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k < K) again(set[2 + k], -(e[k] * is));
        }
    };
    if (clean) {
        ld_row_together<G, M>(wv, qv, lane, ev);
        request(bufA, r + 1);
    }
    for (int l = 0; l + 1 < ECO_LISTS; l += 2) {
        list(bufA, bufB, l);
        list(bufB, bufA, l + 1);
    }
    list(bufA, bufB, ECO_LISTS - 1);
    // W[v] += back_v, after every earlier write of the sample
    if constexpr (MODE == MODE_ATOMIC) {
        atomic_row<G, M>(qv, back, lane, dpad);
    } else {
        if (!clean) {
            eco_wait_memory();
            ld_row_together<G, M>(wv, qv, lane, ev);
        }
#pragma unroll
        for (int m = 0; m < M; ++m) wv[m] = wv[m] + back[m];
        st_row<G, M>(qv, wv, lane, ev);
    }
}

template <int G, int M, int MODE, int KMAX>
__global__ void __launch_bounds__(256) eco_train_kernel(EcoArgs a) {
    const uint64_t RW = (uint64_t)eco_width(a.K);
    const int lane = threadIdx.x & (G - 1);
    const uint64_t gpb = blockDim.x / G, gib = threadIdx.x / G;
    const uint64_t count = a.count;
    bool ev[M];
    row_valid<G, M>(ev, lane, a.dpad);
    unsigned n_clean = 0, n_ordered = 0;   // this group's, since the last counter add
    auto run = [&](uint64_t t) __attribute__((always_inline)) {
        const int32_t* r = a.rec + t * RW;
        if (r[0] < 0) return;   // skipped by the draws
        const unsigned flags = a.clean[t];
        n_clean += flags & 1u;
        n_ordered += !(flags & 1u);
        eco_sample<G, M, MODE, KMAX>(a, lane, ev, r, flags, alpha_at(a.begin + t, a.alpha0, a.total));
    };
    if (a.mode == SMORE_SERIAL) {
        // serial: one group, samples strictly in order
        if (blockIdx.x != 0 || gib != 0) return;
        unsigned long long tc = 0, to = 0;
        for (uint64_t t = 0; t < count; ++t) {
            run(t);
            tc += n_clean;
            to += n_ordered;
            n_clean = n_ordered = 0;
        }
        if (lane == 0) {
            atomicAdd(a.stats, tc);
            atomicAdd(a.stats + 1, to);
        }
        return;
    }
    // chunks of ch_rounds rounds handed out from a.work, as in cbow_train_kernel
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
        // the chunk's counts: one add per wave
        uint32_t cc = lane == 0 ? n_clean : 0u, co = lane == 0 ? n_ordered : 0u;
        n_clean = n_ordered = 0;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            cc += __shfl_xor(cc, m, 64);
            co += __shfl_xor(co, m, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            if (cc) atomicAdd(a.stats, (unsigned long long)cc);
            if (co) atomicAdd(a.stats + 1, (unsigned long long)co);
        }
    }
}

// the (G, M) ladder; a unit (train_eco_<s|a>.hip) exports it as its update_symbol
// specialisations, one per K bucket
template <int KMAX, int MODE>
const void* eco_symbol(int dpad, int) {
    const int G = lanes_of(dpad), M = regs_of(dpad);
#define X(g, m) \
    if (G == g && M == m) return (const void*)eco_train_kernel<g, m, MODE, KMAX>;
    SMORE_FOR_EACH_GM(X)
#undef X
    return nullptr;
}

}  // namespace smore

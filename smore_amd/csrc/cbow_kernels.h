// cbow_kernels.h -- the set-sum (CBOW) update kernel for gfx950 (template): GCN and
// TEXTGCN on table 0 (w_vertex).
//
// proNet::UpdateCBOW (src/proNet.cpp:2868-3001, Opt_SigmoidRegSGD :1332-1351) runs per
// sample, on sets of S = walk_steps row ids:
//   w_avg = sum of the w-set rows (once), c_avg = sum of the c-set rows
//   positive step (label 1): g = label - fastSigmoid(w_avg . c_avg),
//       back_err += alpha (g c_avg - reg w_avg), back_c = alpha (g w_avg - reg c_avg),
//       every c-set row += back_c (an id that occurs twice takes it twice)
//   K negative steps (label 0): the same on a set of S uniform field-1 rows, summed as
//       they are in memory then
//   last, every w-set row += back_err
// Every id comes pre-drawn in the record {vertex, context, c-set[S], w-set[S], K x
// neg-set[S]} (train_cbow_draw.hip), with the sample's clean flag.  DESIGN.md 12e.
//
// One lane group of G lanes per sample (device_common.h row layout).  Only w_avg,
// c_avg, back_err and back_c live for the whole sample.  S and K are run-time
// values, so a set is gathered in batches of B rows (B a compile-time width, the
// tail masked on id -1) into one of two register buffers.  Nothing is written
// before the positive step, so the two positive sets are always requested
// together, batch by batch.  On a clean sample (c-set and negative ids pairwise
// distinct) the next batch of negative rows is requested before the current
// set's dot is reduced and its rows are written: no such row is written earlier
// in the sample.  Otherwise the sample runs in the reference's memory order: a
// set's loads are issued after every earlier add of the sample has completed.
// A write is row += delta: one atomic add of the delta (atomic scatter) or a
// load, an add and a store (plain stores, the serial mode); ids that coincide
// inside a set take it one after the other.  The closing w-set adds wait for
// all the sample's earlier writes.
#pragma once
#include "hoprec_kernels.h"

namespace smore {

template <int G, int M>
__device__ __forceinline__ float cbow_dot(const float (&a)[M], const float (&b)[M]) {
    float p = 0.0f;
#pragma unroll
    for (int m = 0; m < M; ++m) p = __builtin_fmaf(a[m], b[m], p);
    return group_sum<G>(p);
}

// every vector-memory operation of this wave so far (loads, stores, atomic adds) has completed
__device__ __forceinline__ void cbow_wait_memory() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// row q += dl
template <int G, int M, int MODE>
__device__ __forceinline__ void cbow_add(float* q, const float (&dl)[M], int lane, const bool (&ev)[M], int dpad) {
    if constexpr (MODE == MODE_ATOMIC) {
        atomic_row<G, M>(q, dl, lane, dpad);
    } else {
        float row[M];
        ld_row<G, M>(row, q, lane, ev);
#pragma unroll
        for (int m = 0; m < M; ++m) row[m] = row[m] + dl[m];
        st_row<G, M>(q, row, lane, ev);
    }
}

// the set's rows k0 .. k0 + B - 1 (ids -1 from S on) requested together
template <int G, int M, int B>
__device__ __forceinline__ void cbow_gather(float (&row)[B][M], int32_t (&id)[B], const float* T, const int32_t* set,
                                            int k0, int S, int lane, const bool (&ev)[M], int dpad) {
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const int k = k0 + b;
        const int32_t x = set[k < S ? k : 0];
        id[b] = k < S ? x : -1;
    }
#pragma unroll
    for (int b = 0; b < B; ++b) ld_row_together<G, M>(row[b], T + (int64_t)(id[b] < 0 ? 0 : id[b]) * dpad, lane, ev);
}

// acc += the batch's rows, in set order
template <int M, int B>
__device__ __forceinline__ void cbow_sum(float (&acc)[M], const float (&row)[B][M], const int32_t (&id)[B]) {
#pragma unroll
    for (int b = 0; b < B; ++b)
#pragma unroll
        for (int m = 0; m < M; ++m) acc[m] = id[b] >= 0 ? acc[m] + row[b][m] : acc[m];
}

// One sample: record r (cbow_width(a.S, a.K) words) at learning rate alpha.
template <int G, int M, int MODE, int B>
__device__ __forceinline__ void cbow_sample(const CbowArgs& a, const float* s_sig, int lane, const bool (&ev)[M],
                                            const int32_t* r, bool clean, float alpha) {
    const int dpad = a.dpad, S = a.S, K = a.K;
    float* const T = a.T;
    const int32_t* const cset = r + 2;
    const int32_t* const wset = r + 2 + S;
    const int32_t* const nset = r + 2 + 2 * S;
    const int nb = (S + B - 1) / B;   // batches per set
    const int Q = K * nb;             // negative batches of the sample
    const float r_ = alpha * a.reg;
    float w_avg[M], c_avg[M], back[M];
#pragma unroll
    for (int m = 0; m < M; ++m) w_avg[m] = c_avg[m] = back[m] = 0.0f;
    float bufA[B][M], bufB[B][M];
    int32_t idA[B], idB[B];
    // the positive sets: nothing of the sample is written yet
    for (int bi = 0; bi < nb; ++bi) {
        cbow_gather<G, M, B>(bufA, idA, T, cset, bi * B, S, lane, ev, dpad);
        cbow_gather<G, M, B>(bufB, idB, T, wset, bi * B, S, lane, ev, dpad);
        cbow_sum<M, B>(c_avg, bufA, idA);
        cbow_sum<M, B>(w_avg, bufB, idB);
    }
    // the first negative batch: ahead of the positive step when clean, else after its adds
    if (clean) cbow_gather<G, M, B>(bufA, idA, T, nset, 0, S, lane, ev, dpad);
    // a set is complete: the step on c_avg, then the set's rows take back_c
    auto close = [&](const int32_t* set, float label) __attribute__((always_inline)) {
        const float a_ = alpha * (label - fast_sigmoid(cbow_dot<G, M>(w_avg, c_avg), s_sig));
        float bc[M];
#pragma unroll
        for (int m = 0; m < M; ++m) {
            back[m] = __builtin_fmaf(-r_, w_avg[m], __builtin_fmaf(a_, c_avg[m], back[m]));
            bc[m] = __builtin_fmaf(a_, w_avg[m], -(r_ * c_avg[m]));
            c_avg[m] = 0.0f;
        }
        for (int i = 0; i < S; ++i) {
            const int32_t id = set[i];
            if (id >= 0) cbow_add<G, M, MODE>(T + (int64_t)id * dpad, bc, lane, ev, dpad);
        }
    };
    close(cset, 1.0f);
    if (!clean) {
        cbow_wait_memory();
        cbow_gather<G, M, B>(bufA, idA, T, nset, 0, S, lane, ev, dpad);
    }
    // negative batch q (set q / nb, rows (q % nb) B ..) is in `cur`; batch q + 1 goes to `nxt`:
    // ahead of this batch's sum and writes when clean, else after its writes have completed
    auto step = [&](float (&cur)[B][M], int32_t (&icur)[B], float (&nxt)[B][M], int32_t (&inxt)[B],
                    int q) __attribute__((always_inline)) {
        const int k = q / nb, bi = q - k * nb;
        const int k1 = (q + 1) / nb, b1 = q + 1 - k1 * nb;
        const bool more = q + 1 < Q;
        if (clean && more) cbow_gather<G, M, B>(nxt, inxt, T, nset + k1 * S, b1 * B, S, lane, ev, dpad);
        cbow_sum<M, B>(c_avg, cur, icur);
        if (bi == nb - 1) close(nset + k * S, 0.0f);
        if (!clean && more) {
            cbow_wait_memory();
            cbow_gather<G, M, B>(nxt, inxt, T, nset + k1 * S, b1 * B, S, lane, ev, dpad);
        }
    };
    for (int q = 0; q < Q; q += 2) {
        step(bufA, idA, bufB, idB, q);
        if (q + 1 < Q) step(bufB, idB, bufA, idA, q + 1);
    }
    // the w-set last, after every earlier write of the sample
    cbow_wait_memory();
    for (int i = 0; i < S; ++i) {
        const int32_t id = wset[i];
        if (id >= 0) cbow_add<G, M, MODE>(T + (int64_t)id * dpad, back, lane, ev, dpad);
    }
}

template <int G, int M, int MODE, int B>
__global__ void __launch_bounds__(256) cbow_train_kernel(CbowArgs a) {
    __shared__ float s_sig[1001];
    for (int k = threadIdx.x; k < 1001; k += blockDim.x) s_sig[k] = a.sig[k];
    __syncthreads();
    const uint64_t RW = (uint64_t)cbow_width(a.S, a.K);
    const int lane = threadIdx.x & (G - 1);
    const uint64_t gpb = blockDim.x / G, gib = threadIdx.x / G;
    const uint64_t count = a.count;
    bool ev[M];
    row_valid<G, M>(ev, lane, a.dpad);
    unsigned n_clean = 0, n_ordered = 0;   // this group's, since the last counter add
    auto run = [&](uint64_t t) __attribute__((always_inline)) {
        const int32_t* r = a.rec + t * RW;
        if (r[0] < 0) return;   // skipped by the draws
        const bool clean = a.clean[t] != 0;
        n_clean += clean;
        n_ordered += !clean;
        cbow_sample<G, M, MODE, B>(a, s_sig, lane, ev, r, clean, alpha_at(a.begin + t, a.alpha0, a.total));
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

// the (G, M) ladder; a unit (train_cbow_<s|a>.hip) exports it as its update_symbol
// specialisation: KMAX = B, the gather batch
template <int KMAX, int MODE>
const void* cbow_symbol(int dpad, int) {
    const int G = lanes_of(dpad), M = regs_of(dpad);
#define X(g, m) \
    if (G == g && M == m) return (const void*)cbow_train_kernel<g, m, MODE, KMAX>;
    SMORE_FOR_EACH_GM(X)
#undef X
    return nullptr;
}

}  // namespace smore

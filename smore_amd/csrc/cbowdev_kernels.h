// cbowdev_kernels.h -- the bag-of-words event update kernel for gfx950 (template):
// TEXTGCNdev on table 0 (w_vertex) and table 1 (w_context).
//
// proNet::UpdateCBOWdev (src/proNet.cpp:2755-2865, Opt_SigmoidRegSGD :1332-1351) runs per
// sample, E = num_events, N = num_words:
//   w_avg = sum of the E N bag rows of w_context, in order, duplicates counted
//   label = 1; for i < E:
//       step(W[event], w_avg, label -> back_err); step(W[event], W[user], label -> user_err)
//       label = 0; five times: step(W[a], w_avg, 0 -> back_err); step(W[b], W[user], 0 -> user_err)
//   step(row, ctx, label -> acc): g = label - fastSigmoid(row . ctx),
//       row += alpha (g ctx - reg row) in place, then acc += alpha (g row - reg ctx) on the
//       row as just updated
//   last, W[user] += user_err and every bag row += back_err (an id that occurs twice
//   takes it twice)
// `event` is the last event the collection loop drew, and only iteration 0 has label 1:
// the reference's accidents, kept.  Every id comes pre-drawn in the record
// {user, event, bag[E N], E x {a0, b0, .. a4, b4}} (train_cbowdev_draw.hip), with the
// sample's clean flag.
//
// One lane group of G lanes per sample (device_common.h row layout).  w_avg, W[user],
// user_err, back_err and W[event] live for the whole sample.  The bag is gathered in
// batches of B rows as cbow_gather does.  On a clean sample (user, event and the 10 E
// negative ids pairwise distinct) W[user] and W[event] are read once, W[event] stays in
// registers across its 2 E steps, an iteration's ten negative rows are requested together
// and (AHEAD) the next iteration's ten before this iteration's rows are written.  Otherwise
// the sample runs in the reference's memory order: each step's row, and W[user], are read
// after every earlier write of the sample has completed, so a negative equal to `event`,
// repeated negatives and a self-loop event == user come out as in the reference.  A step
// writes row' (plain stores, the serial mode) or adds its delta with one atomic add (atomic
// scatter).  The closing adds wait for all the sample's earlier writes.
#pragma once
#include "cbow_kernels.h"

namespace smore {

// one step on `row` (at q) against ctx; alias: ctx is this very row (event == user), so the
// second half reads it as updated
template <int G, int M, int MODE>
__device__ __forceinline__ void cbowdev_step(float (&row)[M], const float (&ctx)[M], bool alias, float label, float alpha,
                                             float r_, float (&acc)[M], float* q, const float* s_sig, int lane,
                                             const bool (&ev)[M], int dpad) {
    const float a_ = alpha * (label - fast_sigmoid(cbow_dot<G, M>(row, ctx), s_sig));
    float d[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        d[m] = __builtin_fmaf(a_, ctx[m], -(r_ * row[m]));
        row[m] = row[m] + d[m];
        acc[m] = __builtin_fmaf(-r_, alias ? row[m] : ctx[m], __builtin_fmaf(a_, row[m], acc[m]));
    }
    if constexpr (MODE == MODE_ATOMIC) atomic_row<G, M>(q, d, lane, dpad);
    else st_row<G, M>(q, row, lane, ev);
}

// an iteration's ten negative rows requested together
template <int G, int M>
__device__ __forceinline__ void cbowdev_gather10(float (&row)[2 * CBOWDEV_NEG][M], const float* T, const int32_t* neg,
                                                 int lane, const bool (&ev)[M], int dpad) {
#pragma unroll
    for (int n = 0; n < 2 * CBOWDEV_NEG; ++n) ld_row_together<G, M>(row[n], T + (int64_t)neg[n] * dpad, lane, ev);
}

// One sample: record r (cbowdev_width(a.E, a.N) words) at learning rate alpha.
template <int G, int M, int MODE, int B>
__device__ __forceinline__ void cbowdev_sample(const CbowDevArgs& a, const float* s_sig, int lane, const bool (&ev)[M],
                                               const int32_t* r, bool clean, float alpha) {
    constexpr int NN = 2 * CBOWDEV_NEG;
    constexpr bool AHEAD = M == 4;   // two ten-row buffers; at M = 8 one (registers)
    const int dpad = a.dpad, E = a.E, S = a.E * a.N;
    float* const T = a.T;
    float* const Cx = a.C;
    const int32_t user = r[0], event = r[1];
    const int32_t* const bag = r + 2;
    const int32_t* const neg = r + 2 + S;
    float* const qu = T + (int64_t)user * dpad;
    float* const qe = T + (int64_t)event * dpad;
    const float r_ = alpha * a.reg;
    float w_avg[M], back[M], uerr[M], wu[M], we[M];
#pragma unroll
    for (int m = 0; m < M; ++m) w_avg[m] = back[m] = uerr[m] = 0.0f;
    // nothing of the sample is written yet
    ld_row_together<G, M>(wu, qu, lane, ev);
    float nA[NN][M], nB[AHEAD ? NN : 1][M];
    if (clean) {
        // W[event] stays in registers on this path only: the ordered path reads each step's row itself
        ld_row_together<G, M>(we, qe, lane, ev);
        cbowdev_gather10<G, M>(nA, T, neg, lane, ev, dpad);
    }
    {
        float buf[B][M];
        int32_t id[B];
        for (int k0 = 0; k0 < S; k0 += B) {
            cbow_gather<G, M, B>(buf, id, Cx, bag, k0, S, lane, ev, dpad);
            cbow_sum<M, B>(w_avg, buf, id);
        }
    }
    if (clean) {
        // iteration i's negative rows are in `cur`; iteration i + 1's go to `nxt`
        auto iter = [&](float (&cur)[NN][M], float (&nxt)[AHEAD ? NN : 1][M], int i) __attribute__((always_inline)) {
            const float label = i == 0 ? 1.0f : 0.0f;
            const int32_t* const ni = neg + i * NN;
            if constexpr (AHEAD)
                if (i + 1 < E) cbowdev_gather10<G, M>(nxt, T, ni + NN, lane, ev, dpad);
            cbowdev_step<G, M, MODE>(we, w_avg, false, label, alpha, r_, back, qe, s_sig, lane, ev, dpad);
            cbowdev_step<G, M, MODE>(we, wu, false, label, alpha, r_, uerr, qe, s_sig, lane, ev, dpad);
#pragma unroll
            for (int n = 0; n < NN; ++n) {
                float* const q = T + (int64_t)ni[n] * dpad;
                if (n & 1) cbowdev_step<G, M, MODE>(cur[n], wu, false, 0.0f, alpha, r_, uerr, q, s_sig, lane, ev, dpad);
                else cbowdev_step<G, M, MODE>(cur[n], w_avg, false, 0.0f, alpha, r_, back, q, s_sig, lane, ev, dpad);
            }
        };
        if constexpr (AHEAD) {
            for (int i = 0; i < E; i += 2) {
                iter(nA, nB, i);
                if (i + 1 < E) iter(nB, nA, i + 1);
            }
        } else {
            for (int i = 0; i < E; ++i) {
                // the rows are clean: none of them is written by this iteration's two event steps
                if (i > 0) cbowdev_gather10<G, M>(nA, T, neg + i * NN, lane, ev, dpad);
                iter(nA, nB, i);
            }
        }
    } else {
        // the reference's memory order: a step's row, and W[user], after every earlier write
        float row[M];
        bool first = true;
        for (int i = 0; i < E; ++i) {
            for (int q = 0; q < 2 + NN; ++q) {
                const int32_t id = q < 2 ? event : neg[i * NN + q - 2];
                float* const p = T + (int64_t)id * dpad;
                const float label = i == 0 && q < 2 ? 1.0f : 0.0f;
                if (!first) {
                    cbow_wait_memory();
                    if (q & 1) ld_row_together<G, M>(wu, qu, lane, ev);
                }
                first = false;
                ld_row_together<G, M>(row, p, lane, ev);
                if (q & 1) cbowdev_step<G, M, MODE>(row, wu, id == user, label, alpha, r_, uerr, p, s_sig, lane, ev, dpad);
                else cbowdev_step<G, M, MODE>(row, w_avg, false, label, alpha, r_, back, p, s_sig, lane, ev, dpad);
            }
        }
    }
    // the closing writes, after every earlier write of the sample
    cbow_wait_memory();
    cbow_add<G, M, MODE>(qu, uerr, lane, ev, dpad);
    for (int i = 0; i < S; ++i) cbow_add<G, M, MODE>(Cx + (int64_t)bag[i] * dpad, back, lane, ev, dpad);
}

template <int G, int M, int MODE, int B>
__global__ void __launch_bounds__(256) cbowdev_train_kernel(CbowDevArgs a) {
    __shared__ float s_sig[1001];
    for (int k = threadIdx.x; k < 1001; k += blockDim.x) s_sig[k] = a.sig[k];
    __syncthreads();
    const uint64_t RW = (uint64_t)cbowdev_width(a.E, a.N);
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
        cbowdev_sample<G, M, MODE, B>(a, s_sig, lane, ev, r, clean, alpha_at(a.begin + t, a.alpha0, a.total));
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

// the (G, M) ladder; a unit (train_cbowdev_<s|a>.hip) exports it as its update_symbol
// specialisation: KMAX = B, the bag's gather batch
template <int KMAX, int MODE>
const void* cbowdev_symbol(int dpad, int) {
    const int G = lanes_of(dpad), M = regs_of(dpad);
#define X(g, m) \
    if (G == g && M == m) return (const void*)cbowdev_train_kernel<g, m, MODE, KMAX>;
    SMORE_FOR_EACH_GM(X)
#undef X
    return nullptr;
}

}  // namespace smore

// train_hoprec_draw.hip -- the sampling half of HOP-REC (HBPR::Train,
// src/model/HBPR.cpp:94-114, and the in-rule negatives of
// proNet::UpdateFBPRPair, src/proNet.cpp:1474-1483).
//
// None of a sample's draws depends on the tables, so all 1 + 6 walk_steps row
// ids are drawn ahead: one thread per sample walks the sample's Philox unit
// (unit s of stream 0) slot by slot, in the order of the reference's
// random_gen calls, and writes
//     rec[t] = {v, i_1, j_10..j_14, i_2, j_20..j_24, ...}   (tagged ids)
// hoprec_width(steps) words, -1 from the step at which the sample stopped.
//   source attempt         2 slots (p, index), repeated while field[v] != 0
//   TargetSample           2 slots (p, index); a vertex without out-edge: no slot, -1
//   step w > 1             i = TargetSample(TargetSample(i))
//   NegativeSample attempt 2 slots (index, p), repeated while field[j] != field[i]
//   in-rule negative       1 slot per attempt: a uniform index, same rejection
// A rejection loop gives up after HOPREC_ATTEMPTS draws and a TargetSample may
// return -1: the sample stops there (the step is not run, earlier steps are)
// and is counted once in *skipped.
#include "train_kernels.h"

namespace smore {

// the unit's words in slot order, one Philox block per four
struct UnitWords {
    uint64_t seed, unit;
    uint32_t slot = 0, blk = 0xFFFFFFFFu;
    uint32_t w[4];
    __device__ __forceinline__ uint32_t next() {
        if ((slot >> 2) != blk) {
            blk = slot >> 2;
            const uint4 b = philox_block(seed, 0, unit, blk);
            w[0] = b.x;
            w[1] = b.y;
            w[2] = b.z;
            w[3] = b.w;
        }
        return w[slot++ & 3];
    }
};

__global__ void __launch_bounds__(256) hoprec_draw_kernel(DevGraph g, const int32_t* __restrict__ field, uint64_t seed,
                                                          uint64_t begin, uint64_t count, int steps, int32_t* rec,
                                                          uint32_t* slots, unsigned long long* skipped) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int RW = hoprec_width(steps);
    int32_t* const r = rec + t * RW;
    UnitWords u;
    u.seed = seed;
    u.unit = begin + t;
    bool stopped = false;
    // the source: a field-0 vertex (a user)
    int32_t tv = -1;
    for (uint32_t a = 0;; ++a) {
        if (a == HOPREC_ATTEMPTS) {
            stopped = true;
            break;
        }
        const uint32_t kp = u.next(), ki = u.next();
        tv = source_sample(g, kp, ki);
        if (field[untag(tv)] == 0) break;
    }
    r[0] = stopped ? -1 : tv;
    int32_t i = -1;
    if (!stopped) {
        if (g.offsets[untag(tv) + 1] != g.offsets[untag(tv)]) {
            const uint32_t kp = u.next(), ki = u.next();
            i = target_sample(g, untag(tv), kp, ki);
        }
        stopped = i < 0;
    }
    int w = 1;
    for (; w <= steps && !stopped; ++w) {
        int32_t* const o = r + 1 + (1 + HOPREC_NEG) * (w - 1);
        if (w > 1) {
            for (int hop = 0; hop < 2 && i >= 0; ++hop) {
                const int32_t at = untag(i);
                if (g.offsets[at + 1] == g.offsets[at]) {
                    i = -1;
                } else {
                    const uint32_t kp = u.next(), ki = u.next();
                    i = target_sample(g, at, kp, ki);
                }
            }
            if (i < 0) break;
        }
        const int32_t fi = field[untag(i)];
        int32_t j[HOPREC_NEG];
        bool ok = true;
#pragma unroll
        for (int n = 0; n < HOPREC_NEG && ok; ++n) {
            for (uint32_t a = 0;; ++a) {
                if (a == HOPREC_ATTEMPTS) {
                    ok = false;
                    break;
                }
                if (n == 0) {
                    const uint32_t ki = u.next(), kp = u.next();
                    j[n] = negative_sample(g, ki, kp);
                } else {
                    j[n] = (int32_t)draw_index(u.next(), g.V);
                }
                if (field[untag(j[n])] == fi) break;
            }
        }
        if (!ok) break;
        o[0] = i;
#pragma unroll
        for (int n = 0; n < HOPREC_NEG; ++n) o[1 + n] = j[n];
    }
    // w: the first step not written (steps + 1: the sample is complete)
    if (w <= steps) {
        for (int k = 1 + (1 + HOPREC_NEG) * (w - 1); k < 1 + (1 + HOPREC_NEG) * steps; ++k) r[k] = -1;
        atomicAdd(skipped, 1ull);
    }
    for (int k = 1 + (1 + HOPREC_NEG) * steps; k < RW; ++k) r[k] = -1;
    if (slots) slots[t] = u.slot;
}

hipError_t launch_hoprec_draw(const DevGraph& g, const int32_t* field, uint64_t seed, uint64_t begin, uint64_t count,
                              int steps, int32_t* rec, uint32_t* slots, unsigned long long* skipped, hipStream_t st) {
    const int block = 256;
    hipLaunchKernelGGL(hoprec_draw_kernel, dim3((unsigned)((count + block - 1) / block)), dim3(block), 0, st, g, field,
                       seed, begin, count, steps, rec, slots, skipped);
    return hipGetLastError();
}

}  // namespace smore

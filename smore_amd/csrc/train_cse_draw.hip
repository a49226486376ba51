// train_cse_draw.hip -- the sampling half of CSE (NEMF::Train, src/model/NEMF.cpp:119-131,
// NERANK::Train, src/model/NERANK.cpp:119-130, and the draws inside
// proNet::UpdateBatchCommunity, src/proNet.cpp:3149-3168, UpdateFactorizedPair
// :2605-2608 and UpdateUIPair :2632-2638).
//
// None of a sample's draws depends on the tables, so every row id is drawn
// ahead: one thread per sample walks the sample's Philox unit (unit s of stream
// 0) slot by slot, in the order of the reference's random_gen calls, and writes
//     rec[t] = {v, c, A: n_00..n_04, then per step s >= 1 ctx_s, n_s0..n_s4; B: the same; D}
// cse_width(steps, rank) words of plain ids, -1 from where a pass stopped.
//   source attempt          2 slots (p, index), repeated while field[v] != 0
//   TargetSample            2 slots (p, index); a vertex without out-edge: no slot, -1
//   pass A / B, step s > 0  ctx_s = TargetSample(ctx_{s-1}); A starts at v, B at c
//   NegativeSample          2 slots (index, p)
//   nemf direct term        five NegativeSample
//   nerank direct term      sixteen uniform indices, 1 slot per attempt, each repeated while
//                           field[j] != field[c] (the reference stops at the one that passes
//                           its gate; the slots after it are simply unused)
// A rejection loop gives up after CSE_ATTEMPTS draws.  c == -1 (or no field-0
// source) skips the sample; a walk that hits -1 ends that pass only, an
// exhausted nerank loop ends the direct negatives there.  Each such sample is
// counted once in *skipped.
#include "train_kernels.h"

namespace smore {

namespace {
// the unit's words in slot order, one Philox block per four
struct CseWords {
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
}  // namespace

__global__ void __launch_bounds__(256) cse_draw_kernel(DevGraph g, const int32_t* __restrict__ field, uint64_t seed,
                                                       uint64_t begin, uint64_t count, int steps, int rank,
                                                       int32_t* rec, uint32_t* slots, unsigned long long* skipped) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int RW = cse_width(steps, rank), D = cse_dneg(rank);
    int32_t* const r = rec + t * RW;
    CseWords u;
    u.seed = seed;
    u.unit = begin + t;
    for (int k = 0; k < RW; ++k) r[k] = -1;
    // the source: a field-0 vertex (a user), then its target
    int32_t v = -1, c = -1;
    for (uint32_t a = 0; a < CSE_ATTEMPTS; ++a) {
        const uint32_t kp = u.next(), ki = u.next();
        const int32_t x = untag(source_sample(g, kp, ki));
        if (field[x] == 0) {
            v = x;
            break;
        }
    }
    if (v >= 0) {
        r[0] = v;
        if (g.offsets[v + 1] != g.offsets[v]) {
            const uint32_t kp = u.next(), ki = u.next();
            c = target_sample(g, v, kp, ki);
        }
    }
    bool early = c < 0;
    if (c >= 0) {
        c = untag(c);
        r[1] = c;
        for (int p = 0; p < 2; ++p) {
            int32_t* const o = r + 2 + p * (6 * steps - 1);
            int32_t ctx = p == 0 ? v : c;
            for (int st = 0; st < steps; ++st) {
                int32_t* q = o;
                if (st) {
                    if (g.offsets[ctx + 1] == g.offsets[ctx]) {
                        ctx = -1;
                    } else {
                        const uint32_t kp = u.next(), ki = u.next();
                        ctx = untag(target_sample(g, ctx, kp, ki));
                    }
                    if (ctx < 0) {
                        early = true;
                        break;
                    }
                    q = o + CSE_NEG + 6 * (st - 1);
                    *q++ = ctx;
                }
                for (int n = 0; n < CSE_NEG; ++n) {
                    const uint32_t ki = u.next(), kp = u.next();
                    q[n] = untag(negative_sample(g, ki, kp));
                }
            }
        }
        int32_t* const dn = r + 12 * steps;
        const int32_t fc = field[c];
        for (int n = 0; n < D; ++n) {
            if (!rank) {
                const uint32_t ki = u.next(), kp = u.next();
                dn[n] = untag(negative_sample(g, ki, kp));
                continue;
            }
            int32_t j = -1;
            for (uint32_t a = 0; a < CSE_ATTEMPTS; ++a) {
                const int32_t x = (int32_t)draw_index(u.next(), g.V);
                if (field[x] == fc) {
                    j = x;
                    break;
                }
            }
            if (j < 0) {
                early = true;
                break;
            }
            dn[n] = j;
        }
    }
    if (early) atomicAdd(skipped, 1ull);
    if (slots) slots[t] = u.slot;
}

hipError_t launch_cse_draw(const DevGraph& g, const int32_t* field, uint64_t seed, uint64_t begin, uint64_t count,
                           int steps, int rank, int32_t* rec, uint32_t* slots, unsigned long long* skipped,
                           hipStream_t st) {
    const int block = 256;
    hipLaunchKernelGGL(cse_draw_kernel, dim3((unsigned)((count + block - 1) / block)), dim3(block), 0, st, g, field,
                       seed, begin, count, steps, rank, rec, slots, skipped);
    return hipGetLastError();
}

}  // namespace smore

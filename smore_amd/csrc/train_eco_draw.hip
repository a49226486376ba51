// train_eco_draw.hip -- the sampling half of the sampled-softmax (ECO) rule (ECO::Train,
// src/model/ECO.cpp:97-100, and the draws inside proNet::UpdateDChoice,
// src/proNet.cpp:2241-2244 and :2269).
//
// None of a sample's draws depends on the table, so every row id is drawn
// ahead: one thread per sample walks the sample's Philox unit (unit s of stream
// 0) slot by slot, in the order of the reference's random_gen calls, and writes
//     rec[t] = {v, then per list c1, c2, n_0..n_{K-1}}
// eco_width(K) words of plain ids.
//   source attempt    2 slots (p, index), repeated while field[v1] != 0
//   v2                TargetSample(v1), 2 slots; the rule never uses its value
//   per list          c1 = TargetSample(v), x = TargetSample(c1), c2 = TargetSample(x), 2 slots
//                     each; then K x NegativeSample, 2 slots each (index, p)
// The source loop gives up after ECO_ATTEMPTS draws.  A sample one of whose
// TargetSamples returns -1 (a vertex without out-edge; the draws stop there) or
// whose source loop gave up is skipped: its record is all -1 and it is counted
// once in *skipped.  clean[t] bit 0 is set when the sample's 1 + 5 (2 + K) ids are
// pairwise distinct (eco_kernels.h takes those samples' rows together), bit 1 + l
// when v and list l's 2 + K ids are (that list needs no second read of a row).
#include "train_kernels.h"

namespace smore {

namespace {
// the unit's words in slot order, one Philox block per four
struct EcoWords {
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
    // TargetSample(v): -1 and no slot for a vertex without out-edge
    __device__ __forceinline__ int32_t target(const DevGraph& g, int32_t v) {
        if (g.offsets[v + 1] == g.offsets[v]) return -1;
        const uint32_t kp = next(), ki = next();
        return untag(target_sample(g, v, kp, ki));
    }
};
}  // namespace

__global__ void __launch_bounds__(256) eco_draw_kernel(DevGraph g, const int32_t* __restrict__ field, uint64_t seed,
                                                       uint64_t begin, uint64_t count, int K, int32_t* rec,
                                                       uint8_t* clean, uint32_t* slots, unsigned long long* skipped) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int RW = eco_width(K);
    int32_t* const r = rec + t * RW;
    EcoWords u;
    u.seed = seed;
    u.unit = begin + t;
    for (int k = 0; k < RW; ++k) r[k] = -1;
    // the source: a field-0 vertex
    int32_t v = -1;
    for (uint32_t a = 0; a < ECO_ATTEMPTS; ++a) {
        const uint32_t kp = u.next(), ki = u.next();
        const int32_t x = untag(source_sample(g, kp, ki));
        if (field[x] == 0) {
            v = x;
            break;
        }
    }
    bool skip = v < 0;
    if (!skip) skip = u.target(g, v) < 0;   // v2: drawn and thrown away
    if (!skip) r[0] = v;
    for (int l = 0; !skip && l < ECO_LISTS; ++l) {
        int32_t* const o = r + 1 + l * (2 + K);
        const int32_t c1 = u.target(g, v);
        int32_t c2 = c1 < 0 ? -1 : u.target(g, c1);
        if (c2 >= 0) c2 = u.target(g, c2);
        if (c2 < 0) {
            skip = true;
            break;
        }
        o[0] = c1;
        o[1] = c2;
        for (int k = 0; k < K; ++k) {
            const uint32_t ki = u.next(), kp = u.next();
            o[2 + k] = untag(negative_sample(g, ki, kp));
        }
    }
    // bit 0: all ids pairwise distinct; bit 1 + l: v and list l's 2 + K ids pairwise distinct
    unsigned fl = 0;
    if (skip) {
        for (int k = 0; k < RW; ++k) r[k] = -1;
        atomicAdd(skipped, 1ull);
    } else {
        bool cl = true;
        for (int l = 0; l < ECO_LISTS; ++l) {
            const int i0 = 1 + l * (2 + K);
            bool own = true;
            for (int i = i0; i < i0 + 2 + K; ++i) {
                const int32_t x = r[i];
                own = own && x != v;
                for (int j = 1; j < i; ++j)
                    if (r[j] == x) {
                        cl = false;
                        own = own && j < i0;
                    }
            }
            cl = cl && own;
            fl |= own ? 2u << l : 0u;
        }
        fl |= cl ? 1u : 0u;
    }
    clean[t] = (uint8_t)fl;
    if (slots) slots[t] = u.slot;
}

hipError_t launch_eco_draw(const DevGraph& g, const int32_t* field, uint64_t seed, uint64_t begin, uint64_t count,
                           int K, int32_t* rec, uint8_t* clean, uint32_t* slots, unsigned long long* skipped,
                           hipStream_t st) {
    const int block = 256;
    hipLaunchKernelGGL(eco_draw_kernel, dim3((unsigned)((count + block - 1) / block)), dim3(block), 0, st, g, field,
                       seed, begin, count, K, rec, clean, slots, skipped);
    return hipGetLastError();
}

}  // namespace smore

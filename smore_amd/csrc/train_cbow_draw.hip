// train_cbow_draw.hip -- the sampling half of the set-sum (CBOW) rule (GCN::Train,
// src/model/GCN.cpp:93-99, TEXTGCN::Train, src/model/TEXTGCN.cpp:120-126, and the draws
// inside proNet::UpdateCBOW, src/proNet.cpp:2879-2892 and :2954-2960).
//
// None of a sample's draws depends on the table, so every row id is drawn
// ahead: one thread per sample walks the sample's Philox unit (unit s of stream
// 0) slot by slot, in the order of the reference's random_gen calls, and writes
//     rec[t] = {vertex, context, c-set[S], w-set[S], K x neg-set[S]}
// cbow_width(S, K) words of plain ids.
//   source attempt    2 slots (p, index), repeated while field[v1] != 0
//   TEXTGCN's v2      TargetSample(v1), 2 slots; GCN: vertex = context = v1
//   c-set, w-set      S x TargetSample(context), S x TargetSample(vertex), 2 slots each; a
//                     vertex without out-edge takes no slot and its set is S times -1
//   negative set      S uniform indices, 1 slot per attempt, each repeated while field != 1
// A rejection loop gives up after CBOW_ATTEMPTS draws.  A sample without v2,
// with both sets empty or with an exhausted loop is skipped: its record is all
// -1 and it is counted once in *skipped.  clean[t] = 1 when the c-set ids and
// the K S negative ids are pairwise distinct (cbow_kernels.h takes those
// samples' rows together).
#include "train_kernels.h"

namespace smore {

namespace {
// the unit's words in slot order, one Philox block per four
struct CbowWords {
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

__global__ void __launch_bounds__(256) cbow_draw_kernel(DevGraph g, const int32_t* __restrict__ field, uint64_t seed,
                                                        uint64_t begin, uint64_t count, int model, int S, int K,
                                                        int32_t* rec, uint8_t* clean, uint32_t* slots,
                                                        unsigned long long* skipped) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int RW = cbow_width(S, K);
    int32_t* const r = rec + t * RW;
    CbowWords u;
    u.seed = seed;
    u.unit = begin + t;
    for (int k = 0; k < RW; ++k) r[k] = -1;
    // the source: a field-0 vertex
    int32_t v1 = -1, vertex = -1;
    for (uint32_t a = 0; a < CBOW_ATTEMPTS; ++a) {
        const uint32_t kp = u.next(), ki = u.next();
        const int32_t x = untag(source_sample(g, kp, ki));
        if (field[x] == 0) {
            v1 = x;
            break;
        }
    }
    bool skip = v1 < 0;
    if (!skip) {
        vertex = v1;
        if (model == SMORE_CBOW_TEXTGCN) {
            vertex = -1;
            if (g.offsets[v1 + 1] != g.offsets[v1]) {
                const uint32_t kp = u.next(), ki = u.next();
                vertex = untag(target_sample(g, v1, kp, ki));
            }
        }
        skip = vertex < 0;
    }
    if (!skip) {
        r[0] = vertex;
        r[1] = v1;
        for (int p = 0; p < 2; ++p) {
            const int32_t from = p ? vertex : v1;
            if (g.offsets[from + 1] == g.offsets[from]) continue;
            for (int i = 0; i < S; ++i) {
                const uint32_t kp = u.next(), ki = u.next();
                r[2 + p * S + i] = untag(target_sample(g, from, kp, ki));
            }
        }
        skip = r[2] < 0 && r[2 + S] < 0;
    }
    for (int n = 0; !skip && n < K * S; ++n) {
        int32_t j = -1;
        for (uint32_t a = 0; a < CBOW_ATTEMPTS; ++a) {
            const int32_t x = (int32_t)draw_index(u.next(), g.V);
            if (field[x] == 1) {
                j = x;
                break;
            }
        }
        skip = j < 0;
        r[2 + 2 * S + n] = j;
    }
    bool cl = false;
    if (skip) {
        for (int k = 0; k < RW; ++k) r[k] = -1;
        atomicAdd(skipped, 1ull);
    } else {
        // pairwise distinct: the c-set (word 2 ..) and the negatives (word 2 + 2S ..); the w-set
        // between them is left out, and so is an empty c-set's -1
        cl = true;
        const int n = 2 + 2 * S + K * S;
        for (int i = 3; i < n && cl; ++i) {
            if (i >= 2 + S && i < 2 + 2 * S) continue;
            const int32_t x = r[i];
            if (x < 0) continue;
            for (int j = 2; j < i; ++j)
                if ((j < 2 + S || j >= 2 + 2 * S) && r[j] == x) {
                    cl = false;
                    break;
                }
        }
    }
    clean[t] = cl ? 1 : 0;
    if (slots) slots[t] = u.slot;
}

hipError_t launch_cbow_draw(const DevGraph& g, const int32_t* field, uint64_t seed, uint64_t begin, uint64_t count,
                            int model, int S, int K, int32_t* rec, uint8_t* clean, uint32_t* slots,
                            unsigned long long* skipped, hipStream_t st) {
    const int block = 256;
    hipLaunchKernelGGL(cbow_draw_kernel, dim3((unsigned)((count + block - 1) / block)), dim3(block), 0, st, g, field,
                       seed, begin, count, model, S, K, rec, clean, slots, skipped);
    return hipGetLastError();
}

}  // namespace smore

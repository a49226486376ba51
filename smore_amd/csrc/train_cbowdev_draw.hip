// train_cbowdev_draw.hip -- the sampling half of the bag-of-words event rule
// (TEXTGCNdev::Train, src/model/TEXTGCNdev.cpp:103-108, and the draws inside
// proNet::UpdateCBOWdev, src/proNet.cpp:2765-2774 and :2814-2822).
//
// None of a sample's draws depends on a table, so every row id is drawn ahead:
// one thread per sample walks the sample's Philox unit (unit s of stream 0)
// slot by slot, in the order of the reference's random_gen calls, and writes
//     rec[t] = {user, event, bag[E N], E x {a0, b0, .. a4, b4}}
// cbowdev_width(E, N) words of plain ids.
//   source attempt    2 slots (p, index), repeated while field[user] != 0
//   collection        E times: event = TargetSample(user), then N times word =
//                     TargetSample(event); 2 slots each, none for a vertex without
//                     out-edge, where the sample ends.  `event` is the last one drawn
//   negatives         10 E uniform indices, 1 slot per attempt, each repeated while
//                     field != 1
// A rejection loop gives up after CBOWDEV_ATTEMPTS draws.  A sample whose
// collection meets a vertex without out-edge, or with an exhausted loop, is
// skipped: its record is all -1 and it is counted once in *skipped.  clean[t]
// = 1 when user, event and the 10 E negative ids are pairwise distinct
// (cbowdev_kernels.h takes those samples' rows together); the bag ids address
// the other table.
#include "train_kernels.h"

namespace smore {

namespace {
// the unit's words in slot order, one Philox block per four
struct CbowDevWords {
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

__global__ void __launch_bounds__(256) cbowdev_draw_kernel(DevGraph g, const int32_t* __restrict__ field, uint64_t seed,
                                                           uint64_t begin, uint64_t count, int E, int N, int32_t* rec,
                                                           uint8_t* clean, uint32_t* slots, unsigned long long* skipped) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int RW = cbowdev_width(E, N);
    int32_t* const r = rec + t * RW;
    CbowDevWords u;
    u.seed = seed;
    u.unit = begin + t;
    for (int k = 0; k < RW; ++k) r[k] = -1;
    // the source: a field-0 vertex
    int32_t user = -1, event = -1;
    for (uint32_t a = 0; a < CBOWDEV_ATTEMPTS; ++a) {
        const uint32_t kp = u.next(), ki = u.next();
        const int32_t x = untag(source_sample(g, kp, ki));
        if (field[x] == 0) {
            user = x;
            break;
        }
    }
    bool skip = user < 0;
    // the collection: E events, N words of each
    for (int i = 0; !skip && i < E; ++i) {
        skip = g.offsets[user + 1] == g.offsets[user];
        if (skip) break;
        {
            const uint32_t kp = u.next(), ki = u.next();
            event = untag(target_sample(g, user, kp, ki));
        }
        skip = g.offsets[event + 1] == g.offsets[event];
        for (int j = 0; !skip && j < N; ++j) {
            const uint32_t kp = u.next(), ki = u.next();
            r[2 + i * N + j] = untag(target_sample(g, event, kp, ki));
        }
    }
    const int nneg = 2 * CBOWDEV_NEG * E;
    int32_t* const neg = r + 2 + E * N;
    for (int n = 0; !skip && n < nneg; ++n) {
        int32_t j = -1;
        for (uint32_t a = 0; a < CBOWDEV_ATTEMPTS; ++a) {
            const int32_t x = (int32_t)draw_index(u.next(), g.V);
            if (field[x] == 1) {
                j = x;
                break;
            }
        }
        skip = j < 0;
        neg[n] = j;
    }
    bool cl = false;
    if (skip) {
        for (int k = 0; k < RW; ++k) r[k] = -1;
        atomicAdd(skipped, 1ull);
    } else {
        r[0] = user;
        r[1] = event;
        // pairwise distinct: user, event and the negatives
        cl = user != event;
        for (int i = 0; i < nneg && cl; ++i) {
            const int32_t x = neg[i];
            cl = x != user && x != event;
            for (int j = 0; j < i && cl; ++j) cl = neg[j] != x;
        }
    }
    clean[t] = cl ? 1 : 0;
    if (slots) slots[t] = u.slot;
}

hipError_t launch_cbowdev_draw(const DevGraph& g, const int32_t* field, uint64_t seed, uint64_t begin, uint64_t count,
                               int E, int N, int32_t* rec, uint8_t* clean, uint32_t* slots,
                               unsigned long long* skipped, hipStream_t st) {
    const int block = 256;
    hipLaunchKernelGGL(cbowdev_draw_kernel, dim3((unsigned)((count + block - 1) / block)), dim3(block), 0, st, g, field,
                       seed, begin, count, E, N, rec, clean, slots, skipped);
    return hipGetLastError();
}

}  // namespace smore

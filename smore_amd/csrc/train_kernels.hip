// train_kernels.hip -- sampler / init kernels and the resolver of the update
// kernels: update_kernel maps (family, scatter mode, K, dpad, model) to the
// instantiation that one of the train_edge_* / train_pair_* / train_go_rec_*
// / train_warp_* / train_hoprec_* / train_skewopt_* / train_cse_* / train_cbow_* / train_eco_* / train_cbowdev_* units exports (train_kernels.h SMORE_FOR_EACH_UPDATE_KERNEL).

#include "train_kernels.h"

namespace smore {

// ------------------------------------------------------------------ sampler
__global__ void sample_kernel(DevGraph g, uint64_t seed, uint64_t begin, uint64_t count, int K,
                              int bpr, int32_t* out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const uint64_t s = begin + t;
    const int nslot = bpr ? 14 : 4 + 2 * K;
    const int width = bpr ? 7 : 2 + K;
    int32_t* o = out + t * width;
    uint32_t w[4];
    uint32_t blk = 0xFFFFFFFFu;
    auto word = [&](int j) -> uint32_t {
        if ((uint32_t)(j >> 2) != blk) {
            blk = (uint32_t)(j >> 2);
            const uint4 b = philox_block(seed, 0, s, blk);
            w[0] = b.x; w[1] = b.y; w[2] = b.z; w[3] = b.w;
        }
        return w[j & 3];
    };
    (void)nslot;
    const int32_t v = untag(source_sample(g, word(0), word(1)));
    o[0] = v;
    const uint32_t tp = word(2), ti = word(3);
    const int32_t c = target_sample(g, v, tp, ti);
    o[1] = c < 0 ? -1 : untag(c);
    const int nn = bpr ? 5 : K;
    for (int j = 0; j < nn; ++j) {
        const uint32_t ki = word(4 + 2 * j), kp = word(5 + 2 * j);
        o[2 + j] = untag(negative_sample(g, ki, kp));
    }
}

// ------------------------------------------------------------------ init
__global__ void init_uniform_kernel(float* T, int64_t rows, int dim, int dpad, uint64_t seed) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * dpad) return;
    const int64_t v = i / dpad;
    const int d = (int)(i % dpad);
    float x = 0.0f;
    if (d < dim) {
        const uint4 b = philox_block(seed, 2, (uint64_t)v, (uint32_t)(d >> 2));
        const double u = ldexp((double)comp(b, d & 3), -32);
        x = (float)((u - 0.5) / dim);
    }
    T[i] = x;
}

// ------------------------------------------------------------------ dispatch
int lanes_of(int dpad) {
    int nq = (dpad + 3) / 4, G = 1;
    while (G < nq && G < 64) G <<= 1;
    return G;
}

// the instantiation (family, scatter of `mode`, kmax) for dpad and model
static const void* find_symbol(KernelFamily f, int mode, int kmax, int dpad, int model) {
    const int inst = mode == SMORE_ATOMIC ? MODE_ATOMIC : mode == SMORE_HYBRID ? MODE_HYBRID : MODE_STORE;
#define X(F, MODE, KMAX)                                         \
    if (f == KernelFamily::F && inst == MODE && kmax == KMAX)    \
        return update_symbol<KernelFamily::F, MODE, KMAX>(dpad, model);
    SMORE_FOR_EACH_UPDATE_KERNEL(X)
#undef X
    return nullptr;
}

static bool pair_path(const EdgeArgs& a) {
    return a.alpha_rec == 1 && a.mode != SMORE_SERIAL && a.K <= 10 && !a.rec_edge;
}

UpdateKernel update_kernel(UpdateFamily f, const EdgeArgs& a) {
    KernelFamily kf = KernelFamily::Edge;
    int kmax = kmax_of(a.K);
    switch (f) {
        case UpdateFamily::Cpp: kf = pair_path(a) ? KernelFamily::Pair : KernelFamily::Edge; break;
        // the Go kernels have KMAX 5 and 10 (the drivers reject K > 10)
        case UpdateFamily::GoRec: kf = KernelFamily::GoRec; kmax = std::min(kmax, 10); break;
        case UpdateFamily::GoPair: kf = KernelFamily::GoPair; kmax = std::min(kmax, 10); break;
    }
    return {find_symbol(kf, a.mode, kmax, a.dpad, a.model),
            a.mode == SMORE_HYBRID ? sh_lds_bytes(a.sh_rows, a.dpad) : 0};
}

// SMORE_ATOMIC runs the atomic scatter, every other mode the plain stores
UpdateKernel update_kernel(const WarpArgs& a) {
    const int mode = a.mode == SMORE_ATOMIC ? SMORE_ATOMIC : SMORE_HOGWILD;
    return {find_symbol(KernelFamily::Warp, mode, WARP_KMAX, a.dpad, 0), 0};
}

UpdateKernel update_kernel(const HopRecArgs& a) {
    const int mode = a.mode == SMORE_ATOMIC ? SMORE_ATOMIC : SMORE_HOGWILD;
    return {find_symbol(KernelFamily::HopRec, mode, HOPREC_KMAX, a.dpad, 0), 0};
}

UpdateKernel update_kernel(const SkewOptArgs& a) {
    const int mode = a.mode == SMORE_ATOMIC ? SMORE_ATOMIC : SMORE_HOGWILD;
    return {find_symbol(KernelFamily::SkewOpt, mode, SKEWOPT_KMAX, a.dpad, 0), 0};
}

UpdateKernel update_kernel(const CseArgs& a) {
    const int mode = a.mode == SMORE_ATOMIC ? SMORE_ATOMIC : SMORE_HOGWILD;
    return {find_symbol(KernelFamily::Cse, mode, cse_dneg(a.rank), a.dpad, 0), 0};
}

UpdateKernel update_kernel(const CbowArgs& a) {
    const int mode = a.mode == SMORE_ATOMIC ? SMORE_ATOMIC : SMORE_HOGWILD;
    return {find_symbol(KernelFamily::Cbow, mode, CBOW_BATCH, a.dpad, 0), 0};
}

UpdateKernel update_kernel(const EcoArgs& a) {
    const int mode = a.mode == SMORE_ATOMIC ? SMORE_ATOMIC : SMORE_HOGWILD;
    return {find_symbol(KernelFamily::Eco, mode, kmax_of(a.K), a.dpad, 0), 0};
}

UpdateKernel update_kernel(const CbowDevArgs& a) {
    const int mode = a.mode == SMORE_ATOMIC ? SMORE_ATOMIC : SMORE_HOGWILD;
    return {find_symbol(KernelFamily::CbowDev, mode, CBOWDEV_BATCH, a.dpad, 0), 0};
}

hipError_t launch_sample(const DevGraph& g, uint64_t seed, uint64_t begin, uint64_t count, int K,
                         int bpr, int32_t* out, hipStream_t st) {
    const int block = 256;
    const uint64_t grid = (count + block - 1) / block;
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)grid), dim3(block), 0, st, g, seed, begin, count, K,
                       bpr, out);
    return hipGetLastError();
}

hipError_t launch_init_uniform(float* T, int64_t rows, int dim, int dpad, uint64_t seed, hipStream_t st) {
    const int64_t n = rows * dpad;
    const int block = 256;
    hipLaunchKernelGGL(init_uniform_kernel, dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, st, T,
                       rows, dim, dpad, seed);
    return hipGetLastError();
}

}  // namespace smore

/* exp32.h -- the one fp32 exponential of the sampled-softmax (ECO) rule, shared
 * bit for bit by the kernel (eco_kernels.h) and the CPU spec (tests/c/eco_spec.c).
 * The C library's and the device library's expf differ in their last bits, so
 * the rule's exponential is defined here from operations that IEEE fixes:
 * +, *, fmaf, float <-> int conversion and a bit cast.  Compiles as C and as
 * HIP; both sides build with -ffp-contract=off.
 *
 *   z = x * log2(e), n = z rounded to the nearest integer (half away from zero)
 *   r = x - n ln2, ln2 split in two (0.693359375 exact in 9 bits, -2.12194440e-4)
 *   p = 1 + r + r^2 P(r), P of degree 5 (the Cephes expf coefficients), |r| <= 0.3466
 *   result = p with n added to its exponent field (p in [0.70, 1.42], n in [-124, 127])
 *
 * Outside fp32's range: x > 88 gives +inf (exp(88) = 1.65e38 is the largest
 * value returned from the polynomial; expf overflows from 88.72); x < -86
 * gives +0 (exp(-86) = 4.5e-38 is still a normal number; no result is ever
 * subnormal); a NaN is returned as it is.
 * Relative error against double exp over 10^6 evenly spaced arguments of
 * [-20, 20]: DESIGN.md 12f. */
#ifndef SMORE_EXP32_H
#define SMORE_EXP32_H

#if defined(__HIPCC__) || defined(__HIP__)
#define SMORE_EXP32_FN __host__ __device__ static inline
#define SMORE_EXP32_FMA(a, b, c) __builtin_fmaf(a, b, c)
#else
#include <math.h>
#define SMORE_EXP32_FN static inline
#define SMORE_EXP32_FMA(a, b, c) fmaf(a, b, c)
#endif

SMORE_EXP32_FN float exp32(float x) {
    if (x != x) return x;
    if (x > 88.0f) return __builtin_inff();
    if (x < -86.0f) return 0.0f;
    const float z = x * 1.44269504088896341f;
    const int n = (int)(z + (z < 0.0f ? -0.5f : 0.5f));
    const float nf = (float)n;
    float r = SMORE_EXP32_FMA(nf, -0.693359375f, x);
    r = SMORE_EXP32_FMA(nf, 2.12194440e-4f, r);
    float p = 1.9875691500e-4f;
    p = SMORE_EXP32_FMA(p, r, 1.3981999507e-3f);
    p = SMORE_EXP32_FMA(p, r, 8.3334519073e-3f);
    p = SMORE_EXP32_FMA(p, r, 4.1665795894e-2f);
    p = SMORE_EXP32_FMA(p, r, 1.6666665459e-1f);
    p = SMORE_EXP32_FMA(p, r, 5.0000001201e-1f);
    p = SMORE_EXP32_FMA(p, r * r, r) + 1.0f;
    union {
        float f;
        int i;
    } u;
    u.f = p;
    u.i += n * (1 << 23);
    return u.f;
}

#endif

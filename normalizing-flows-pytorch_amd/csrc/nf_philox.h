// Counter-based random numbers shared by the kernels that draw on the device: Philox4x32-10 (stateless: the same counter and key always
// give the same four words) and Box-Muller normals in float32.  Used by datagen.hip (synthetic batches) and cnf.hip (Hutchinson noise).
#pragma once
#include "nf_common.h"

struct NfPhilox { unsigned c[4]; };
__device__ __forceinline__ NfPhilox nf_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
    const unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += W0; k1 += W1;
    }
    NfPhilox o;
    o.c[0] = c0; o.c[1] = c1; o.c[2] = c2; o.c[3] = c3;
    return o;
}
// (0, 1): 23 random bits + a half -- (float)(x >> 9) + 0.5f is exact for every x (no round-up to 1.0 at the top of the range)
__device__ __forceinline__ float nf_u01(unsigned x) { return ((float)(x >> 9) + 0.5f) * (1.f / 8388608.f); }
__device__ __forceinline__ void nf_box_muller(unsigned a, unsigned b, float& n0, float& n1) {
    const float r = sqrtf(-2.f * logf(nf_u01(a))), t = 6.283185307179586f * nf_u01(b);
    n0 = r * cosf(t);
    n1 = r * sinf(t);
}

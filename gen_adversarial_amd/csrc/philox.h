// The counter-based generator behind ga_randn and the NES kernels (include/ga_ops.h states the numbers, gen_adversarial_amd/noise.py
// restates them): Philox4x32-10 on four counter words under a two-word key, the exact fp32 uniforms of its output words, and
// Box-Muller on the two pairs.  One copy: every kernel that draws includes this header, so every kernel draws the same normals.
#pragma once
#include "ga_common.h"

namespace ga {

constexpr unsigned PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&x)[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const unsigned hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
    x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

// u = ((x >> 9) + 0.5) * 2^-23: the sum needs 24 bits, so every step is exact; 2^-24 <= u <= 1 - 2^-24
__device__ __forceinline__ float uniform01(unsigned x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }

// the four unit normals of four output words.  logf / sqrtf / sincospif are the library's accurate forms (the fast v_log_f32 path
// loses 1e-6 relative near u = 1, where ln u is tiny): the kernels wait on their stores either way.
__device__ __forceinline__ floatx4 box_muller_quad(const unsigned (&x)[4]) {
    floatx4 v;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float rad = sqrtf(-2.0f * logf(uniform01(x[2 * j])));
        float sn, cs;
        sincospif(2.0f * uniform01(x[2 * j + 1]), &sn, &cs);
        v[2 * j] = rad * cs;
        v[2 * j + 1] = rad * sn;
    }
    return v;
}

// key (k0, k1), counter (c0, c1, c2, c3) = (quad, row, tensor, draw) -> the unit normals of elements 4 c0 .. 4 c0 + 3 of that row
__device__ __forceinline__ floatx4 philox_normal_quad(unsigned k0, unsigned k1, unsigned c0, unsigned c1, unsigned c2, unsigned c3) {
    unsigned x[4];
    philox4x32_10(c0, c1, c2, c3, k0, k1, x);
    return box_muller_quad(x);
}

}  // namespace ga

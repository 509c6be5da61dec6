// The split-bf16 operand path shared by the dense kernels (conv_bf3, conv_halo3, conv_thin3, conv_pw_frag, the fused decoder
// cells): prologue on a channel quad, bf16 hi / lo split, the three-MFMA product, the XCD tile order and the key of the
// instantiated prologue variants.  Each kernel keeps what is its own: where scale / shift come from, its padding predicate, its
// LDS addressing and its scheduling hints.  (See conv_bf3.hip for why three bf16 MFMAs give fp32-class products.)
#pragma once
#include "ga_common.h"

namespace ga {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

// ---- prologue, in the order every kernel applies it: affine (AFF == 1: pro_affine4; AFF == 2: v * scale + shift of the row),
//      activation, then the kernel's own padding select (act(0) = 0 for all of them: only a shift un-zeroes padding)

// AFF == 1: per-channel scale / shift, or nn.PReLU (GA_CONV_PRO_PRELU, uniform: the slopes travel in pro_scale)
__device__ __forceinline__ floatx4 pro_affine4(floatx4 v, const floatx4 rs, const floatx4 rt, const bool prelu) {
    if (prelu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * rs[e];
    } else {
        v = v * rs + rt;
    }
    return v;
}

template <int ACT>
__device__ __forceinline__ floatx4 pro_act4(floatx4 v) {
    if (ACT == GA_ACT_SILU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] * fast_sigmoid(v[e]);
    } else if (ACT == GA_ACT_ELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : __expf(v[e]) - 1.f;
    } else if (ACT == GA_ACT_RELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
    } else if (ACT == GA_ACT_LRELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.01f * v[e];
    }
    return v;
}

// ---- operand split: v = hi + lo + r, hi = bf16(v), lo = bf16(v - hi)
__device__ __forceinline__ void split4(const floatx4 v, bf16x4& hi, bf16x4& lo) {
    hi = __builtin_convertvector(v, bf16x4);
    lo = __builtin_convertvector(v - __builtin_convertvector(hi, floatx4), bf16x4);
}

// two quads into one 8-wide fragment (same values as two split4; both hi parts first, the order the decoder cells were scheduled with)
__device__ __forceinline__ void split8(const floatx4 a, const floatx4 b, bf16x8& hi, bf16x8& lo) {
    const bf16x4 ha = __builtin_convertvector(a, bf16x4), hb = __builtin_convertvector(b, bf16x4);
    const bf16x4 la = __builtin_convertvector(a - __builtin_convertvector(ha, floatx4), bf16x4);
    const bf16x4 lb = __builtin_convertvector(b - __builtin_convertvector(hb, floatx4), bf16x4);
    hi = __builtin_shufflevector(ha, hb, 0, 1, 2, 3, 4, 5, 6, 7);
    lo = __builtin_shufflevector(la, lb, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ---- THE summation order of the library: per 16-deep k step acc += a_lo b_hi, then a_hi b_lo, then a_hi b_hi (small terms
//      first), k ascending.  Every kernel that claims bitwise agreement with another one (tile 8 = tiles 5 - 7, tile 11 = tile 7,
//      tile 12 = tiles 1 - 4, fused cells = unfused launches) does so because both sum through this function, in the same k order.
__device__ __forceinline__ void mfma3(floatx16& acc, const bf16x8 ah, const bf16x8 al, const bf16x8 bh, const bf16x8 bl) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}

// ---- logical tile of this workgroup: blockIdx.x is dealt round-robin to the 8 XCDs, so consecutive logical tiles (which share
//      the A panel) are given to the workgroups of ONE XCD, i.e. one L2
__device__ __forceinline__ int xcd_tile_id() {
    const int nb = gridDim.x, orig = blockIdx.x;
    const int q = nb >> 3, r = nb & 7, xcd = orig & 7, k = orig >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

// ---- host: (affine kind << 4) | activation, the key of the instantiated prologue variants (conv_bf3 adds its dual bit)
inline int conv_pro_mode(const ga_conv_desc& d) {
    return ((d.pro_scale ? (d.pro_per_row ? 2 : 1) : 0) << 4) | d.pro_act;
}

// The prologues of the 3x3 halo kernels (conv_halo3 tiles 5 - 8, conv_thin3): X(mode, AFF, ACT, WIDE).  WIDE: tiles 5 - 7 also
// have the 13-slot row-segment kernel for it — none (backward convs), the per-channel affine / PReLU (e4e IR units at 256^2 and
// 128^2) and the per-row style scale (StyleGAN2 modulated convs).  The first two are what the quick experiment builds keep.
#define GA_CONV3_MODES_EXP(X)      \
    X(0x00, 0, GA_ACT_NONE, true)  \
    X(0x01, 0, GA_ACT_SILU, false)
#define GA_CONV3_MODES(X)          \
    GA_CONV3_MODES_EXP(X)          \
    X(0x02, 0, GA_ACT_ELU, false)  \
    X(0x03, 0, GA_ACT_RELU, false) \
    X(0x04, 0, GA_ACT_LRELU, false) \
    X(0x10, 1, GA_ACT_NONE, true)  \
    X(0x11, 1, GA_ACT_SILU, false) \
    X(0x20, 2, GA_ACT_NONE, true)
#define GA_MODE_CASE(MODE, ...) case MODE:
inline int conv3_mode_supported(const ga_conv_desc& d) {
    switch (conv_pro_mode(d)) {
        GA_CONV3_MODES(GA_MODE_CASE) return 1;
        default: return 0;
    }
}

}  // namespace ga

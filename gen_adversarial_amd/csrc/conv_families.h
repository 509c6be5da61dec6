// The host-side contract between ga_conv2d (conv2d.hip) and the convolution kernel families: one check and one launch per family,
// declared here and nowhere else.  Every family file includes this header, so a signature that drifts is a compile error.
#pragma once
#include "ga_common.h"

namespace ga {

// What ga_conv2d has established about a validated descriptor before it asks a family: the tile code (the heuristic's when the
// caller passed 0), whether the inputs / the output side can be accessed as float4 (vec / vec_out), whether the split-bf16
// operands are usable (bf3: w_hi / w_lo given and aligned, the fast loaders' extents, a prologue conv_bf3 instantiates) and
// the split-K factor after clamping (1 = none).
struct conv_req { int tile, vec, vec_out, bf3, splits; };

// conv_<family>_check: GA_OK when the family takes (d, r) on r.tile, else the refusal code.  The WHOLE answer for the family's
//     tile codes — shape, prologue, LDS bounds, w_frag, splits, vec_out, bf3; launches nothing and calls no HIP API.
//     engine_core's *_ok predicates restate these functions one to one.
// conv_<family>_launch: computes the geometry and enqueues; precondition check(d, r) == GA_OK.  d carries the buffer extents
//     (x_bytes / x2_bytes / w_bytes) ga_conv2d filled in.
#define GA_CONV_FAMILY(NAME)                                           \
    int conv_##NAME##_check(const ga_conv_desc& d, const conv_req& r); \
    int conv_##NAME##_launch(const ga_conv_desc& d, const conv_req& r, hipStream_t stream);
GA_CONV_FAMILY(mfma)        // conv_mfma.hip:    tiles 1 - 4, fp32 MFMA: takes every validated descriptor
GA_CONV_FAMILY(bf3)         // conv_bf3.hip:     tiles 1 - 4 on the split-bf16 operands
GA_CONV_FAMILY(halo3)       // conv_halo3.hip:   tiles 5 - 7 (LDS-staged weights), 8 (weight fragments from w_frag)
GA_CONV_FAMILY(quad3)       // conv_quad3.hip:   tile 9
GA_CONV_FAMILY(thin3)       // conv_thin3.hip:   tile 11
GA_CONV_FAMILY(pw_frag)     // conv_pw_frag.hip: tile 12
#undef GA_CONV_FAMILY

// predicates one file owns and another needs
int conv_bf3_mode_ok(const ga_conv_desc& d);        // conv_bf3.hip: a kernel exists for the prologue / dual-source combination (part of bf3)
int conv_halo3_shape_ok(const ga_conv_desc& d);     // conv_halo3.hip: 3x3 / stride 1 / pad 1 on 128-pixel row tiles (tile 9 builds on it)

// The launch geometry the implicit-GEMM families share: BM x BN output tiles over M = N * Ho * Wo pixels and Cout channels,
// grid.y = split-K slices, and dynamic LDS for the larger of the K loop's buffers and the epilogue's [BM][BN + 4] staging tile.
struct conv_tiling { int M, tilesM, tilesN; dim3 grid; size_t lds; };
inline conv_tiling conv_tile_grid(const ga_conv_desc& d, const int BM, const int BN, const int splits, const size_t lds_kernel) {
    conv_tiling t;
    t.M = d.N * d.Ho * d.Wo;
    t.tilesM = (t.M + BM - 1) / BM;
    t.tilesN = (d.Cout + BN - 1) / BN;
    t.grid = dim3(t.tilesM * t.tilesN, splits);
    const size_t lds_epilogue = (size_t)BM * (BN + 4) * sizeof(float);
    t.lds = lds_kernel > lds_epilogue ? lds_kernel : lds_epilogue;
    return t;
}

}  // namespace ga

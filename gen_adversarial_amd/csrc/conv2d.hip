// ga_conv2d — the host entry of the convolutions: validates the descriptor, cuts tensors past 2 GB into row sub-batches, works
// out what the operands allow (float4 access, the split-bf16 path), picks a tile when the caller named none, hands the
// descriptor to the kernel family that owns the tile code (conv_families.h) and, for split-K, sums the partial tiles.  No
// convolution kernel lives here: each family's file holds its kernels, its check and its launch.
// Also ga_split_bf16, the weight-preparation helper of the split-bf16 families.
#include "conv_epilogue.h"
#include "conv_families.h"

namespace ga {

// sums the split-K partial tiles in split order (bitwise reproducible) and applies the epilogue
__global__ void __launch_bounds__(256) conv_splitk_reduce_kernel(const ga_conv_desc d, const int M, const int splits, const int vec_out) {
    const int HoWo = d.Ho * d.Wo;
    const size_t slab = (size_t)M * d.Cout;
    if (vec_out) {
        const long total4 = (long)slab / 4;
        const int C4 = d.Cout / 4;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
            floatx4 v = *reinterpret_cast<const floatx4*>(d.ws + i * 4);
            for (int s = 1; s < splits; ++s) v += *reinterpret_cast<const floatx4*>(d.ws + s * slab + i * 4);
            epilogue4(d, (int)(i / C4), (int)(i % C4) * 4, v, HoWo);
        }
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < (long)slab; i += (long)gridDim.x * 256) {
            float v = d.ws[i];
            for (int s = 1; s < splits; ++s) v += d.ws[s * slab + i];
            epilogue1(d, (int)(i / d.Cout), (int)(i % d.Cout), v, HoWo);
        }
    }
}

// host helper exported for weight preparation: w (fp32, n elements) -> hi, lo (bf16 bit patterns)
__global__ void split_bf16_kernel(const float* w, __bf16* hi, __bf16* lo, const long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float v = w[i];
        const __bf16 h = (__bf16)v;
        hi[i] = h;
        lo[i] = (__bf16)(v - (float)h);
    }
}

// Who takes which tile codes, in the order ga_conv2d asks.  A code two families list (1 - 4) goes to the first whose check
// accepts; a code nobody lists (10, 13, ...) is refused.  A new family is one line here and one GA_CONV_FAMILY in the header.
struct conv_family {
    int tile_lo, tile_hi;
    int (*check)(const ga_conv_desc&, const conv_req&);
    int (*launch)(const ga_conv_desc&, const conv_req&, hipStream_t);
};
static const conv_family CONV_FAMILIES[] = {
    {1, 4, conv_bf3_check, conv_bf3_launch},            // the heuristic's tiles on the split-bf16 operands when they are usable,
    {1, 4, conv_mfma_check, conv_mfma_launch},          // else on the exact fp32 kernel
    {5, 8, conv_halo3_check, conv_halo3_launch},        // explicit requests only from here on: the tune table names them per shape
    {9, 9, conv_quad3_check, conv_quad3_launch},
    {11, 11, conv_thin3_check, conv_thin3_launch},
    {12, 12, conv_pw_frag_check, conv_pw_frag_launch},
};

static int validate(const ga_conv_desc& d) {
    if (!d.x || !d.w || !d.y) return GA_E_BADARG;
    if (d.N <= 0 || d.Hi <= 0 || d.Wi <= 0 || d.C1 <= 0 || d.C2 < 0 || d.Ho <= 0 || d.Wo <= 0 || d.Cout <= 0) return GA_E_BADARG;
    if (d.KH <= 0 || d.KW <= 0 || d.sn <= 0 || d.sd <= 0 || d.pad < 0) return GA_E_BADARG;
    if (d.sd & (d.sd - 1)) return GA_E_UNSUPPORTED;          // transposed stride must be a power of two
    if (d.C2 > 0 && !d.x2) return GA_E_BADARG;
    if ((d.pro_scale == nullptr) != (d.pro_shift == nullptr)) return GA_E_BADARG;
    if (d.dact_x && ((d.dact_scale == nullptr) != (d.dact_shift == nullptr))) return GA_E_BADARG;
    if (d.ldx < d.C1 || (d.C2 > 0 && d.ldx2 < d.C2) || d.ldy < d.Cout) return GA_E_BADARG;
    if (d.addend && d.ldadd < d.Cout) return GA_E_BADARG;
    if (d.addend2 && d.ldadd2 < d.Cout) return GA_E_BADARG;
    if (d.dact_x && d.lddact < d.Cout) return GA_E_BADARG;
    if (d.dact_x && d.dact_rep > 1 && d.N % d.dact_rep) return GA_E_BADARG;
    return GA_OK;
}

// byte extent of one operand above which ga_conv2d convolves row sub-batches (the fast loaders' 31-bit offsets); lowered by
// ga_debug_set_conv_row_limit so that tests reach the sub-batch path at small sizes
static long g_conv_row_limit = 0x7fffff00L;

// what ga_conv2d decides about a descriptor before it launches (conv_resolve, below)
struct conv_choice { ga_conv_desc k; conv_req r; const conv_family* family; long M; };
static int conv_resolve(const ga_conv_desc& d, conv_choice* out);

// Rows are independent: a tensor beyond the fast loader's 31-bit byte offsets (2 GB; StyleGAN2's 1024^2 x 32-channel maps
// at a few dozen rows) is convolved in sub-batches of rows that fit, each an ordinary launch on the same stream.
// Returns false when d needs no cutting; else rc is the call's result.
static bool run_in_row_batches(const ga_conv_desc& d, void* stream, int& rc) {
    const long row_x = (long)d.Hi * d.Wi * d.ldx * 4, row_x2 = d.C2 > 0 ? (long)d.Hi * d.Wi * d.ldx2 * 4 : 0;
    long row_max = row_x > row_x2 ? row_x : row_x2;
    const long pix_out = (long)d.Ho * d.Wo * 4;          // every per-row operand counts: output, addends, act' source
    if (pix_out * d.ldy > row_max) row_max = pix_out * d.ldy;
    if (d.addend && !d.addend_bcast_n && pix_out * d.ldadd > row_max) row_max = pix_out * d.ldadd;
    if (d.addend2 && pix_out * d.ldadd2 > row_max) row_max = pix_out * d.ldadd2;
    if (d.dact_x && pix_out * d.lddact > row_max) row_max = pix_out * d.lddact;
    const long lim = g_conv_row_limit;
    if (!(d.N > 1 && row_max * d.N >= lim && row_max < lim)) return false;
    int sub = (int)((lim - 1) / row_max);
    const int arep = d.addend && !d.addend_bcast_n && d.addend_rep > 1 ? d.addend_rep : 1;
    const int drep = d.dact_x && d.dact_rep > 1 ? d.dact_rep : 1;
    const long both = (long)arep * drep;             // operands shared by consecutive rows: cut at their row boundaries
    if (arep > 1 || drep > 1) {                      // (a common multiple; the two never meet on one launch in practice)
        if (d.N % arep || d.N % drep) { rc = GA_E_BADARG; return true; }
        sub -= (int)(sub % both);
        if (sub < both) { rc = GA_E_UNSUPPORTED; return true; }
    }
    // The explicit tiles have a row granularity of their own (tile 9: whole groups of 32 images, tile 12: whole 128-pixel tiles).  A
    // cut on a multiple of 128 rows keeps both for any Ho * Wo, in the sub-batches and in the remainder of an N that had it: a
    // descriptor a family takes at a small N is not refused for its size.  Rows so large that fewer than 128 fit keep the cut above
    // (documented with ga_conv2d in ga_ops.h).
    if (sub >= 128 * both) sub -= (int)(sub % (128 * both));
    // Among the fields that differ between sub-batches a refusal depends on the row count alone (the pointers advance by whole rows
    // of pitches that keep their 16-byte class): ask for the two row counts there are before anything is enqueued, so that a call
    // that returns an error has written nothing
    for (const int n : {sub, d.N % sub}) {
        ga_conv_desc s = d;
        s.N = n;
        if (n > 0 && (rc = conv_resolve(s, nullptr)) != GA_OK) return true;
    }
    for (int n0 = 0; n0 < d.N; n0 += sub) {
        ga_conv_desc s = d;
        s.N = d.N - n0 < sub ? d.N - n0 : sub;
        const size_t pin = (size_t)n0 * d.Hi * d.Wi, pout = (size_t)n0 * d.Ho * d.Wo;
        s.x = d.x + pin * d.ldx;
        if (d.x2) s.x2 = d.x2 + pin * d.ldx2;
        s.y = d.y + pout * d.ldy;
        if (d.addend && !d.addend_bcast_n) s.addend = d.addend + (size_t)(n0 / arep) * d.Ho * d.Wo * d.ldadd;
        if (d.addend2) s.addend2 = d.addend2 + pout * d.ldadd2;
        if (d.dact_x) s.dact_x = d.dact_x + (size_t)(n0 / drep) * d.Ho * d.Wo * d.lddact;
        if (d.pro_scale && d.pro_per_row) {
            s.pro_scale = d.pro_scale + (size_t)n0 * d.C1;
            s.pro_shift = d.pro_shift + (size_t)n0 * d.C1;
        }
        rc = ga_conv2d(&s, stream);
        if (rc != GA_OK) return true;
    }
    rc = GA_OK;
    return true;
}

// the 31-bit pixel / K indices of the kernels, and the split-K factor: the workspace it needs, clamped to the K tiles there are
static int split_factor(const ga_conv_desc& d, int& splits) {
    if ((long)d.N * d.Ho * d.Wo > 0x7fffffffL) return GA_E_UNSUPPORTED;
    if ((long)d.KH * d.KW * (d.C1 + d.C2) > 0x7fffffffL) return GA_E_UNSUPPORTED;
    splits = d.splits <= 1 ? 1 : d.splits;
    if (splits > 1) {
        if (!d.ws || d.ws_floats < (long)splits * d.N * d.Ho * d.Wo * d.Cout) return GA_E_BADARG;
        const int T = d.KH * d.KW * ((d.C1 + d.C2 + 31) / 32);
        if (splits > T) splits = T;
        if (splits > 65535) return GA_E_UNSUPPORTED;
    }
    return GA_OK;
}

// vec / vec_out / bf3 of the request, and into k the buffer extents for the FAST loaders (0 = tensor too large for 31-bit byte
// offsets -> generic loader)
static conv_req operand_classes(const ga_conv_desc& d, const int splits, ga_conv_desc& k) {
    const bool vec = (d.C1 % 4 == 0) && (d.C2 % 4 == 0) && (d.ldx % 4 == 0) && (d.C2 == 0 || d.ldx2 % 4 == 0) &&
                     aligned16(d.x) && aligned16(d.w) && (d.C2 == 0 || aligned16(d.x2)) &&
                     (!d.pro_scale || (aligned16(d.pro_scale) && aligned16(d.pro_shift)));
    const bool vec_out = (d.Cout % 4 == 0) && (d.ldy % 4 == 0) && aligned16(d.y) && (!d.bias || aligned16(d.bias)) &&
                         (!d.addend || (d.ldadd % 4 == 0 && aligned16(d.addend))) &&
                         (!d.addend2 || (d.ldadd2 % 4 == 0 && aligned16(d.addend2))) &&
                         (!d.dact_x || (d.lddact % 4 == 0 && aligned16(d.dact_x) &&
                                        (!d.dact_scale || (aligned16(d.dact_scale) && aligned16(d.dact_shift))))) &&
                         (splits == 1 || aligned16(d.ws));
    const long xb = ((long)d.N * d.Hi * d.Wi - 1) * d.ldx * 4 + (long)d.C1 * 4;
    const long x2b = d.C2 > 0 ? ((long)d.N * d.Hi * d.Wi - 1) * d.ldx2 * 4 + (long)d.C2 * 4 : 0;
    const long wb = (long)d.Cout * d.KH * d.KW * (d.C1 + d.C2) * 4;
    const long lim = 0x7fffff00L;
    k.x_bytes = xb < lim ? (unsigned)xb : 0;
    k.x2_bytes = x2b < lim ? (unsigned)x2b : 0;
    k.w_bytes = wb < lim ? (unsigned)wb : 0;
    const int Ctot = d.C1 + d.C2;
    const bool bf3 = d.w_hi && d.w_lo && vec && d.sd == 1 && (d.C2 == 0 || d.C1 % 32 == 0) && (Ctot % 8 == 0) &&
                     d.KH * d.KW <= 32 && k.x_bytes > 0 && k.w_bytes > 0 && (d.C2 == 0 || k.x2_bytes > 0) &&
                     aligned16(d.w_hi) && aligned16(d.w_lo) && conv_bf3_mode_ok(d);
    return conv_req{d.tile, vec, vec_out, bf3, splits};
}

// the tile of a caller that names none (tile 0): the largest of 128 x 128, 128 x 64 and 64 x 64 that still fills the device
static int heuristic_tile(const ga_conv_desc& d, const long M) {
    if (d.Cout <= 32) return 4;
    if (d.Cout <= 64) return (M >= 128 * 256) ? 2 : 3;
    const long b128 = ((M + 127) / 128) * ((d.Cout + 127) / 128);
    const long b12864 = ((M + 127) / 128) * ((d.Cout + 63) / 64);
    if (b128 >= 512) return 1;
    if (b12864 >= 512) return 2;
    return 3;
}

static int reduce_split_k(const ga_conv_desc& k, const long M, const conv_req& r, hipStream_t stream) {
    long items = M * k.Cout / (r.vec_out ? 4 : 1);
    long blocks = (items + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(conv_splitk_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, k, (int)M, r.splits, r.vec_out);
    return check_launch();
}

// everything ga_conv2d decides about a descriptor that needs no cutting, without enqueuing: the split-K factor, the operand
// classes, the tile and the family whose check accepts it (out, when given); the refusal code otherwise
static int conv_resolve(const ga_conv_desc& d, conv_choice* out) {
    int splits = 1;
    int rc = split_factor(d, splits);
    if (rc != GA_OK) return rc;
    conv_choice c;
    c.M = (long)d.N * d.Ho * d.Wo;
    c.k = d;
    c.r = operand_classes(d, splits, c.k);
    if (c.r.tile == 0) c.r.tile = heuristic_tile(d, c.M);
    rc = GA_E_UNSUPPORTED;
    for (const conv_family& f : CONV_FAMILIES) {
        if (c.r.tile < f.tile_lo || c.r.tile > f.tile_hi) continue;
        if ((rc = f.check(c.k, c.r)) != GA_OK) continue;
        c.family = &f;
        break;
    }
    if (rc == GA_OK && out) *out = c;
    return rc;
}

}  // namespace ga

extern "C" long ga_debug_set_conv_row_limit(long bytes) {
    const long old = ga::g_conv_row_limit;
    ga::g_conv_row_limit = bytes > 0 ? bytes : 0x7fffff00L;
    return old;
}

extern "C" int ga_conv2d(const ga_conv_desc* dp, void* stream_) {
    ga::clear_stale_error();
    using namespace ga;
    if (!dp) return GA_E_BADARG;
    const ga_conv_desc& d = *dp;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    int rc = validate(d);
    if (rc != GA_OK) return rc;
    if (run_in_row_batches(d, stream_, rc)) return rc;
    conv_choice c;
    if ((rc = conv_resolve(d, &c)) != GA_OK) return rc;
    rc = c.family->launch(c.k, c.r, stream);
    if (rc != GA_OK || c.r.splits == 1) return rc;
    return reduce_split_k(c.k, c.M, c.r, stream);
}

extern "C" int ga_split_bf16(const float* w, void* hi, void* lo, long n, void* stream) {
    ga::clear_stale_error();
    if (!w || !hi || !lo || n <= 0) return GA_E_BADARG;
    long blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(ga::split_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w,
                       (__bf16*)hi, (__bf16*)lo, n);
    return ga::check_launch();
}

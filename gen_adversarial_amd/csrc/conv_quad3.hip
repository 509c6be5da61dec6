// conv_quad3 — the QUADRANT TILE (tile code 9): 3x3 / stride 1 / pad 1 convolutions on 4 x 4 images, the third form of the
// conv_halo3_bd structure (conv_halo3.hip: patch staged once per 32-channel chunk, weight fragments read from `w_frag` a tap
// ahead, waves 1 x 4 over the 128 output channels, one barrier per chunk), which never multiplies the zero frame.
//
// On a 4 x 4 image with pad 1 only 100 of the 144 (pixel, tap) pairs read a pixel of the image: 4 taps at a corner, 6 at an edge,
// 9 inside.  Tile 8's 128-pixel tile is 8 whole images in natural order, so each 32-row M tile holds every position and issues
// every tap.  Here a workgroup's 128 output pixels are ONE 2 x 2 QUADRANT OF 32 CONSECUTIVE IMAGES, and each of its four 32-row
// M tiles is one pixel position across the 32 images: whether tap (kh, kw) reads inside the image is then the same for all 32
// rows of an M tile, a compile-time property of (quadrant, position, tap).  Every quadrant holds one corner, two edge and one
// interior position, so every workgroup issues 4 + 6 + 6 + 9 = 25 of the 36 (M tile, tap) groups per chunk: the launch stays
// balanced.  M tile mt of the launch is quadrant mt & 3 of images 32 (mt >> 2) .. + 31: as many M tiles as tile 8 has, the same
// XCD tile order.
//
// Patch: the 3 x 3 block of input pixels the quadrant touches (rows qy .. qy + 2, columns qx .. qx + 2 of the image), for 32
// images: 9 input pixels per 4 outputs, no zero frame — the skipped taps are exactly the ones that would have read it.  LDS
// image of a plane (hi or lo): [9 pixels][32 images][32 channels] bf16, 64 bytes per image, NO padding: the 16-byte piece s of
// image r is stored at piece s ^ ((r >> 2) & 3).  An A-fragment ds_read_b128 reads one piece s of the 32 images of one pixel
// (lanes 32 .. 63: piece s + 1).  The hardware serves it in the 16-lane groups {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31}: the
// images of either group cover every residue r mod 16 once, and r = 4 a + b lands on 16-byte slot 4 b + (s ^ a) of the 256-byte
// bank row — b picks the quarter, a the piece in it: 16 different slots, conflict-free (checked by enumerating both groups for
// s = 0 .. 3; an 80-byte pitch is conflict-free as well but does not leave room for two buffers).  The 8-byte staging writes of
// 16 consecutive lanes (2 images x 8 channel quads) fill two whole 64-byte rows.  A buffer (hi + lo) is 36 KB: the patch is
// always double-buffered in 72 KB, two workgroups per CU.
//
// Prologue and split run once per staged element through conv_split.h; a thread owns one (image, channel quad) and its 9 pixels,
// so the scale / shift of a chunk are one float4 pair per thread, fetched with the patch (per channel, or per (image, channel)).
// Summation order per output element: chunk-major, tap ascending, k ascending, through mfma3 — tile 8's order with the products
// of the zero frame left out.  Those are exact +0.0 or -0.0 terms: the result is tile 8's except that an accumulator that was
// -0.0 before a skipped +0.0 product stays -0.0 (equal as floats, not as bits).
#include <utility>
#include "conv_split.h"
#include "conv_epilogue.h"
#include "conv_families.h"

namespace ga {

namespace {

constexpr int QK = 32;                  // channels per chunk
constexpr int QPIX = 32 * 64;           // bytes of one patch pixel in a plane: 32 images x 32 bf16
constexpr int QPLANE = 9 * QPIX;        // one plane (hi or lo)
constexpr int QBUF = 2 * QPLANE;        // one buffer: hi, then lo

// (quadrant Q = 2 qy + qx, position i = 2 py + px in it, tap = 3 kh + kw) -> pixel 3 ry + rx of the patch, or -1 when the tap reads
// the zero frame.  Output row 2 qy + py reads input row 2 qy + py - 1 + kh = patch row qy + py - 1 + kh.
constexpr int quad_pix(const int Q, const int i, const int tap) {
    const int ry = (Q >> 1) + (i >> 1) - 1 + tap / 3, rx = (Q & 1) + (i & 1) - 1 + tap % 3;
    return (ry >= 0 && ry <= 2 && rx >= 0 && rx <= 2) ? 3 * ry + rx : -1;
}
constexpr int quad_nvalid(const int Q, const int tap) {      // M tiles that take the tap: 1, 2 or 4
    int n = 0;
    for (int i = 0; i < 4; ++i) n += quad_pix(Q, i, tap) >= 0;
    return n;
}
// the MFMA groups of a chunk, in issue order: tap ascending, k step, then the M tiles that take the tap two at a time
struct quad_group { int tap, ks, i0, i1; bool first, last; };       // i1 = -1: one M tile; first / last group of its (tap, k step)
constexpr quad_group quad_group_at(const int Q, const int g) {
    int n = 0;
    for (int tap = 0; tap < 9; ++tap)
        for (int ks = 0; ks < 2; ++ks) {
            int v[4] = {-1, -1, -1, -1}, nv = 0;
            for (int i = 0; i < 4; ++i)
                if (quad_pix(Q, i, tap) >= 0) v[nv++] = i;
            for (int k = 0; k < nv; k += 2, ++n)
                if (n == g) return quad_group{tap, ks, v[k], k + 1 < nv ? v[k + 1] : -1, k == 0, k + 2 >= nv};
        }
    return quad_group{-1, 0, -1, -1, false, false};
}
constexpr int quad_ngroups(const int Q) {
    int n = 0;
    while (quad_group_at(Q, n).tap >= 0) ++n;
    return n;
}
constexpr int quad_mfma3(const int Q) {                      // mfma3 per chunk and k step
    int n = 0;
    for (int t = 0; t < 9; ++t) n += quad_nvalid(Q, t);
    return n;
}
static_assert(quad_mfma3(0) == 25 && quad_mfma3(1) == 25 && quad_mfma3(2) == 25 && quad_mfma3(3) == 25, "4 + 6 + 6 + 9 per quadrant");
static_assert(quad_ngroups(0) == 26 && quad_ngroups(1) == 26 && quad_ngroups(2) == 26 && quad_ngroups(3) == 26, "13 groups per k step");

template <int I> using ic = std::integral_constant<int, I>;
template <class F, int... Is>
__device__ __forceinline__ void static_for(F&& f, std::integer_sequence<int, Is...>) { (f(ic<Is>{}), ...); }

template <int AFF, int ACT>
__global__ void __launch_bounds__(256, 2)
conv_quad3_kernel(const ga_conv_desc d, const int tilesN, const int M, const int C, const int nkc) {
    constexpr int WM = 1, WN = 4, TM = 4, TN = 1, BN = 128;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char* const sm = reinterpret_cast<char*>(smem);
    const int bid = xcd_tile_id();
    const int mt = bid / tilesN, nt = bid % tilesN, n0 = nt * BN;
    const int quad = mt & 3, qy = quad >> 1, qx = quad & 1;
    const int n_first = (mt >> 2) * 32;                      // (a batch of fewer than 32 images is one partial group: images >= N load
                                                             // zeros past the buffer's extent and the epilogue drops their rows, m >= M)

    const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;
    const int img = tid >> 3, c4 = tid & 7;                  // staging: this thread's image and channel quad, all 9 pixels
    const int lrow = lane & 31, lh = lane >> 5;              // fragment lane map: row (= image), k octet of a 16-deep step

    const __amdgpu_buffer_rsrc_t rsrcX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.x), 0, d.x_bytes, 0x00020000);
    const int pixb = d.ldx * 4;                              // bytes between input pixels
    const int gbase = (((n_first + img) * 4 + qy) * 4 + qx) * pixb + c4 * 16;     // patch pixel (0, 0) of the image
    const int wbase = img * 64 + (((c4 >> 1) ^ ((img >> 2) & 3)) << 4) + ((c4 & 1) << 3);
    const size_t prow = AFF == 2 ? (size_t)min(n_first + img, d.N - 1) * C : 0;
    const float* const ptab_s = AFF ? d.pro_scale + prow + 4 * c4 : nullptr;
    const float* const ptab_t = AFF ? d.pro_shift + prow + 4 * c4 : nullptr;
    int rd[2];                                               // A fragment of k step ks: byte offset in a pixel of a plane
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) rd[ks] = lrow * 64 + (((2 * ks + lh) ^ ((lrow >> 2) & 3)) << 4);

    const int splits = gridDim.y, split = blockIdx.y;        // split-K over channel chunks
    const int cper = (nkc + splits - 1) / splits;
    const int cb = split * cper, ce = min(nkc, cb + cper);

    floatx4 rpat[9], rs = {1.f, 1.f, 1.f, 1.f}, rt = {0.f, 0.f, 0.f, 0.f};
    auto issue_patch = [&](const int chunk) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 9; ++j)
            rpat[j] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(rsrcX, gbase, chunk * QK * 4 + ((j / 3) * 4 + j % 3) * pixb, 0));
        if (AFF != 0) {
            rs = *reinterpret_cast<const floatx4*>(ptab_s + chunk * QK);
            rt = *reinterpret_cast<const floatx4*>(ptab_t + chunk * QK);
        }
    };
    auto finish_patch = [&](const int buf) __attribute__((always_inline)) {
        char* const Ph = sm + buf * QBUF + wbase;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            floatx4 v = rpat[j];
            if (AFF == 1) v = pro_affine4(v, rs, rt, d.flags & GA_CONV_PRO_PRELU);
            if (AFF == 2) v = v * rs + rt;
            v = pro_act4<ACT>(v);
            if (AFF != 0) {             // tiles 5 - 8 select the zero padding here, between the activation's multiply and the split's
#pragma unroll                          // subtraction: the product is rounded to fp32 before the split.  Keep that rounding (without
                for (int e = 0; e < 4; ++e) {       // this the compiler contracts v * sigmoid(v) - hi into one fma and lo moves by its last bits)
                    float ve = v[e];
                    asm volatile("" : "+v"(ve));
                    v[e] = ve;
                }
            }
            bf16x4 hi, lo;
            split4(v, hi, lo);
            *reinterpret_cast<bf16x4*>(Ph + j * QPIX) = hi;
            *reinterpret_cast<bf16x4*>(Ph + j * QPIX + QPLANE) = lo;
        }
    };

    // weight fragments of (chunk, tap): 4 x 16 bytes per lane (k step 0 / 1 x hi / lo), lane-linear 1-KB pieces (tile 8's copy)
    const uintx4* wf = reinterpret_cast<const uintx4*>(d.w_frag) + ((size_t)nt * nkc * 9 * 4 + wn) * 4 * 64 + lane;
    uintx4 bcur[4], bnxt[4];
    auto load_B = [&](uintx4 (&b)[4], const int chunk, const int tap, const int ks) __attribute__((always_inline)) {       // hi | lo of one k step
        const uintx4* p = wf + (size_t)(chunk * 9 + tap) * (4 * 4 * 64);
#pragma unroll
        for (int q = 2 * ks; q < 2 * ks + 2; ++q) b[q] = p[q * 64];
    };

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][0][r] = 0.f;

    if (cb < ce) {
        issue_patch(cb);
        load_B(bcur, cb, 0, 0);
        load_B(bcur, cb, 0, 1);
        finish_patch(0);
        __builtin_amdgcn_sched_barrier(0);                   // (the second chunk's loads stay behind the first one's conversion: 36 registers, not 72)
        if (cb + 1 < ce) issue_patch(cb + 1);
    }
    __syncthreads();

    // The K loop of quadrant Q: straight-line per chunk.  A group = (tap, k step, up to two of the M tiles that take the tap): one
    // mfma3 per M tile, 13 groups per k step, 26 per chunk.  As in tile 8 the fragment reads of group g + 1 go out before the MFMAs
    // of group g, but into two register sets of TWO M tiles (32 registers, not 64: with them, the 9 patch slots and both weight sets
    // the kernel keeps its 256 registers without scratch); the next tap's weights are loaded a tap ahead (a k step at a time), and the next chunk's patch
    // is converted into the other buffer behind the MFMAs of the middle of the chunk.
    auto run = [&](auto QC) __attribute__((always_inline)) {
        constexpr int Q = decltype(QC)::value;
        constexpr int NG = quad_ngroups(Q);
        bf16x8 ahs[2][2], als[2][2];
        int buf = 0;
#pragma unroll 1
        for (int chunk = cb; chunk < ce; ++chunk) {
            const char* const pa[2] = {sm + buf * QBUF + rd[0], sm + buf * QBUF + rd[1]};
            auto load_A = [&](auto GC) __attribute__((always_inline)) {
                constexpr int g = decltype(GC)::value;
                constexpr quad_group G = quad_group_at(Q, g);
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int i = k ? G.i1 : G.i0;
                    if (i >= 0) {
                        ahs[g & 1][k] = *reinterpret_cast<const bf16x8*>(pa[G.ks] + quad_pix(Q, i, G.tap) * QPIX);
                        als[g & 1][k] = *reinterpret_cast<const bf16x8*>(pa[G.ks] + quad_pix(Q, i, G.tap) * QPIX + QPLANE);
                    }
                }
            };
            load_A(ic<0>{});
            static_for([&](auto GC) __attribute__((always_inline)) {
                constexpr int g = decltype(GC)::value;
                constexpr quad_group G = quad_group_at(Q, g);
                constexpr int n = G.i1 >= 0 ? 2 : 1;
                if constexpr (G.first) {
                    // the next tap's weight fragments of this k step fly for a whole tap's MFMAs (the last tap of the last chunk re-reads
                    // its own); a k step at a time: the second pair takes the registers the first k step of this tap has released
                    load_B(bnxt, G.tap == 8 ? min(chunk + 1, ce - 1) : chunk, G.tap == 8 ? 0 : G.tap + 1, G.ks);
                    __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
                }
                if constexpr (g + 1 < NG) {
                    load_A(ic<g + 1>{});
                    __builtin_amdgcn_sched_group_barrier(0x100, 2 * (quad_group_at(Q, g + 1).i1 >= 0 ? 2 : 1), 0);       // next group's fragment reads first ...
                }
                const bf16x8 bh = __builtin_bit_cast(bf16x8, bcur[2 * G.ks]), bl = __builtin_bit_cast(bf16x8, bcur[2 * G.ks + 1]);
                mfma3(acc[G.i0][0], ahs[g & 1][0], als[g & 1][0], bh, bl);
                if constexpr (n == 2) mfma3(acc[G.i1][0], ahs[g & 1][1], als[g & 1][1], bh, bl);
                __builtin_amdgcn_sched_group_barrier(0x008, 3 * n, 0);                                                  // ... then this group's MFMAs
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (g == NG / 2) {
                    if (chunk + 1 < ce) {                    // the next chunk's patch into the other buffer, behind the MFMAs
                        finish_patch(buf ^ 1);
                        if (chunk + 2 < ce) issue_patch(chunk + 2);
                    }
                }
                if constexpr (G.ks == 1 && G.last) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) bcur[q] = bnxt[q];
                }
            }, std::make_integer_sequence<int, NG>{});
            __syncthreads();                                 // the other buffer is complete, nobody reads this one any more
            buf ^= 1;
        }
    };
    switch (quad) {                                          // uniform over the workgroup
        case 0: run(ic<0>{}); break;
        case 1: run(ic<1>{}); break;
        case 2: run(ic<2>{}); break;
        default: run(ic<3>{}); break;
    }

    // accumulator row 32 i + r = position i of the quadrant in image n_first + r
    const int mq = n_first * 16 + (2 * qy) * 4 + 2 * qx;
    auto mrow = [&](const int r) __attribute__((always_inline)) { return mq + (r & 31) * 16 + ((r >> 6) << 2) + ((r >> 5) & 1); };
    conv_epilogue_rows<WM, WN, TM, TN>(d, acc, smem, mrow, n0, M, 1, splits, split);      // (vector output is a precondition of the tile)
}

template <int AFF, int ACT>
void launch_quad_inst(const ga_conv_desc& d, hipStream_t stream, dim3 grid, size_t lds, int tilesN, int M, int nkc) {
    static dyn_lds_cache attr;
    (void)ensure_dyn_lds(attr, reinterpret_cast<const void*>(&conv_quad3_kernel<AFF, ACT>), lds);
    hipLaunchKernelGGL((conv_quad3_kernel<AFF, ACT>), grid, dim3(256), lds, stream, d, tilesN, M, d.C1, nkc);
}

}  // namespace

// GA_OK when ga_conv2d takes d on tile 9: the split-bf16 operands and vector output, what the halo kernels take (3x3 / stride 1 /
// pad 1, one source of C1 % 32 == 0 channels, an instantiated prologue), 4 x 4 images in whole groups of 32 (or one partial group:
// N < 32), the fragment-ordered weights of tile 8, split-K over whole chunks
int conv_quad3_check(const ga_conv_desc& d, const conv_req& r) {
    if (!(r.bf3 && r.vec_out && conv_halo3_shape_ok(d)) || d.Hi != 4 || d.Wi != 4 || (d.N % 32 != 0 && d.N > 32)) return GA_E_UNSUPPORTED;
    return d.w_frag && aligned16(d.w_frag) && r.splits <= d.C1 / QK ? GA_OK : GA_E_UNSUPPORTED;
}

int conv_quad3_launch(const ga_conv_desc& d, const conv_req& r, hipStream_t stream) {
    constexpr int BM = 128, BN = 128;
    const int nkc = d.C1 / QK;
    // two patch buffers; the epilogue's [128][132] floats fit in them
    static_assert(2 * QBUF >= BM * (BN + 4) * sizeof(float) && 2 * QBUF <= 80 * 1024, "two workgroups per CU");
    conv_tiling t = conv_tile_grid(d, BM, BN, r.splits, 2 * QBUF);
    t.tilesM = 4 * ((d.N + 31) / 32);       // four quadrant tiles per group of 32 images, a partial group included (= N * 16 / 128
    t.grid.x = t.tilesM * t.tilesN;         // for whole groups: tile 8's count)
#define GA_QUAD(MODE, A, C, WIDE) \
    case MODE: launch_quad_inst<A, C>(d, stream, t.grid, t.lds, t.tilesN, t.M, nkc); break;
    switch (conv_pro_mode(d)) {
        GA_CONV3_MODES(GA_QUAD)
        default: return GA_E_UNSUPPORTED;
    }
#undef GA_QUAD
    return check_launch();
}

}  // namespace ga

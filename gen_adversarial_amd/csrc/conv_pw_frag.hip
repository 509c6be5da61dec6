// conv_pw_frag — 1x1 / stride 1 / pad 0 convolutions (and their transposes, which the engine expresses as 1x1 convolutions) on the
// split-bf16 matrix path, as the ONE-TAP case of conv_halo3_bd_kernel (tile code 8): tile code 12.
//
// conv_bf3 hands every 32-deep weight step registers -> LDS -> waves and converts the activation operand in its loader, between the
// MFMAs it competes with: one barrier per 24 MFMAs per wave.  Here, as on tile 8,
//   * a workgroup owns 128 consecutive pixels x 128 output channels, its four waves are 1 x 4 over the channels: a wave's B fragments
//     are nobody else's and come straight from global memory in fragment order, a 32-channel group ahead, as coalesced 1-KB wave loads
//     (`w_frag`: [N tile][32-channel group][wave][k step][hi | lo][lane][8 bf16], WeightStore.frag3(w, taps=1));
//   * the activation tile of a 128-channel chunk is staged into LDS once per workgroup — prologue (per-channel / per-row affine,
//     SiLU) and bf16 hi / lo split applied on the way — from registers that were loaded a chunk ahead: 96 MFMAs per wave between the
//     two barriers of a chunk boundary (single-buffered: 69,632 B, two workgroups per CU; the co-resident workgroup covers the
//     staging).  The last chunk may be shallower (32, 64 or 96 channels; a channel count that is 16 mod 32 is zero-padded, in LDS
//     and in `w_frag`);
//   * one fragment register set, refilled tile by tile: the two ds_read_b128 of M tile i for the next k step follow the three MFMAs
//     that consumed them (9 MFMAs before their next use).
// Per output element the products are summed chunk-major, k ascending, each through mfma3 (conv_split.h) — the order of conv_bf3:
// results are bitwise those of tiles 1 - 4.  No split-K, one source, pixel counts that are multiples of 128.
#include "conv_split.h"
#include "conv_epilogue.h"
#include "conv_families.h"

namespace ga {

constexpr int PK = 128;         // channels per chunk
constexpr int PLD = PK + 8;     // bf16 per LDS pixel row: 272 B, the 16 rows of a ds_read_b128 lane group fall on 16 distinct 16-B slots
constexpr int PSL = 16;         // float4 slots per thread and chunk: 128 pixels x 32 channel quads / 256 threads

template <int AFF, int ACT>
__global__ void __launch_bounds__(256, 2)
conv_pw_frag_kernel(const ga_conv_desc d, const int tilesN, const int M, const int C, const int nk32, const int vec_out,
                    const fastdiv fd_howo) {
    constexpr int BM = 128, BN = 128;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __bf16* Ph = reinterpret_cast<__bf16*>(smem);           // [128 pixels][PLD] hi, then lo

    const int bid = xcd_tile_id();
    const int m0 = (bid / tilesN) * BM;
    const int nt = bid % tilesN, n0 = nt * BN;

    const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;
    const int lrow = lane & 31, lh = lane >> 5;
    // staging: thread -> channel quad c4 of the chunk and the 16 consecutive pixels 16 prow .. 16 prow + 15 of the tile (one image
    // where the prologue is per row: Ho * Wo is a multiple of 16 then)
    const int c4 = tid & 31, prow = tid >> 5;
    constexpr int INV = 0x7fffffff;
    const __amdgpu_buffer_rsrc_t rsrcX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.x), 0, d.x_bytes, 0x00020000);
    const int xbase = (m0 + prow * PSL) * d.ldx * 4 + c4 * 16;
    const int xstep = d.ldx * 4;
    const int prow_img = AFF == 2 ? fd_div(m0 + prow * PSL, fd_howo) : 0;
    __bf16* const Sh = Ph + prow * PSL * PLD + 4 * c4;

    floatx4 rpat[PSL], rs = {1.f, 1.f, 1.f, 1.f}, rt = {0.f, 0.f, 0.f, 0.f};
    bool sval = false;                                      // the staged quad lies below C (else: zero padding of the last group)
    auto issue_stage = [&](const int chunk) __attribute__((always_inline)) {
        const int c = chunk * PK + 4 * c4;
        sval = c < C;
        const int voff = sval ? xbase : INV;                // (one address register: pixel and chunk travel in the scalar offset)
#pragma unroll
        for (int j = 0; j < PSL; ++j)
            rpat[j] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(rsrcX, voff, chunk * PK * 4 + j * xstep, 0));
        if (AFF != 0) {
            const size_t po = sval ? (size_t)prow_img * C + c : 0;
            rs = *reinterpret_cast<const floatx4*>(d.pro_scale + po);
            rt = *reinterpret_cast<const floatx4*>(d.pro_shift + po);
        }
    };
    auto finish_stage = [&]() __attribute__((always_inline)) {
        const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < PSL; ++j) {
            floatx4 v = rpat[j];
            if (AFF == 1) v = pro_affine4(v, rs, rt, d.flags & GA_CONV_PRO_PRELU);
            if (AFF == 2) v = v * rs + rt;
            v = pro_act4<ACT>(v);
            if (AFF != 0) v = sval ? v : zero;              // only a shift un-zeroes the padding
            bf16x4 hi, lo;
            split4(v, hi, lo);
            *reinterpret_cast<bf16x4*>(Sh + j * PLD) = hi;
            *reinterpret_cast<bf16x4*>(Sh + BM * PLD + j * PLD) = lo;
        }
    };

    // weight fragments of one 32-channel group: 4 x 16 bytes per lane ([k step][hi | lo]), lane-linear 1-KB pieces of `w_frag`.
    // A caller without the fragment copy (w_frag null) gets the same fragments gathered from w_hi / w_lo — 16 bytes per lane from
    // 32 weight rows, the slower path: same bits
    const bool fragw = d.w_frag != nullptr;
    const uintx4* wf = reinterpret_cast<const uintx4*>(d.w_frag) + ((size_t)nt * nk32 * 4 + wn) * 4 * 64 + lane;
    const __amdgpu_buffer_rsrc_t rsrcWh = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(d.w_hi), 0, d.w_bytes / 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrcWl = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(d.w_lo), 0, d.w_bytes / 2, 0x00020000);
    const int wrow = n0 + wn * 32 + lrow;
    const int wvoff = wrow < d.Cout ? (wrow * C + 8 * lh) * 2 : INV;
    uintx4 bcur[4], bnxt[4];
    auto load_B = [&](uintx4 (&b)[4], const int c32) __attribute__((always_inline)) {
        if (fragw) {
            const uintx4* p = wf + (size_t)c32 * (4 * 4 * 64);
#pragma unroll
            for (int q = 0; q < 4; ++q) b[q] = p[q * 64];
        } else {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int k0 = c32 * 32 + ks * 16;          // (the second k step of a half group is zero padding)
                const int vo = k0 < C ? wvoff : INV;
                b[2 * ks] = __builtin_amdgcn_raw_buffer_load_b128(rsrcWh, vo, k0 * 2, 0);
                b[2 * ks + 1] = __builtin_amdgcn_raw_buffer_load_b128(rsrcWl, vo, k0 * 2, 0);
            }
        }
    };

    floatx16 acc[4][1];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][0][r] = 0.f;

    bf16x8 ah[4], al[4];
    const __bf16* const Ah = Ph + lrow * PLD + 8 * lh;
    auto load_A = [&](const __bf16* a, const int i, const int koff) __attribute__((always_inline)) {
        ah[i] = *reinterpret_cast<const bf16x8*>(a + i * 32 * PLD + koff);
        al[i] = *reinterpret_cast<const bf16x8*>(a + BM * PLD + i * 32 * PLD + koff);
    };
    // the 24 MFMAs of the 32-channel group whose fragments start at `a`; `more` (a literal at the call sites): another group of
    // this chunk follows, its first fragments are read behind the last MFMAs of this one
    auto group = [&](const __bf16* a, const bool more) __attribute__((always_inline)) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 bh = __builtin_bit_cast(bf16x8, bcur[2 * ks]), bl = __builtin_bit_cast(bf16x8, bcur[2 * ks + 1]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                mfma3(acc[i][0], ah[i], al[i], bh, bl);
                if (ks == 0 || more) load_A(a, i, (ks + 1) * 16);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) bcur[q] = bnxt[q];
    };

    const int nchunks = (nk32 + 3) >> 2;
    issue_stage(0);
    load_B(bcur, 0);
    finish_stage();
    __syncthreads();
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        const int ng = min(4, nk32 - chunk * 4);            // 4 for every chunk that has a successor
        const bool next = chunk + 1 < nchunks;
#pragma unroll
        for (int i = 0; i < 4; ++i) load_A(Ah, i, 0);
        // ONE path for full and shallow chunks (two would make the accumulators meet in phi copies): a loop over all groups but the
        // last, then the last.  The next group's weights leave first; the next chunk's activation loads leave in group 1, behind
        // them: the counted wait for the weights of group 2 does not cover them, and they have two more groups to land
#pragma unroll 1
        for (int g = 0; g + 1 < ng; ++g) {
            load_B(bnxt, chunk * 4 + g + 1);
            __builtin_amdgcn_sched_barrier(0);
            if (g == 1 && next) {
                issue_stage(chunk + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            group(Ah + g * 32, true);
        }
        load_B(bnxt, min(chunk * 4 + ng, nk32 - 1));        // (the last group of the last chunk re-reads its own)
        __builtin_amdgcn_sched_barrier(0);
        group(Ah + (ng - 1) * 32, false);
        if (next) {
            __syncthreads();                                // every wave has read the chunk
            finish_stage();
            __syncthreads();
        }
    }
    __syncthreads();
    conv_epilogue<1, 4, 4, 1>(d, acc, smem, m0, n0, M, vec_out, 1, 0);
}

template <int AFF, int ACT>
static void launch_pw_frag_inst(const ga_conv_desc& d, hipStream_t stream, dim3 grid, size_t lds, int tilesN, int M, int nk32,
                                int vec_out) {
    static dyn_lds_cache attr;
    (void)ensure_dyn_lds(attr, reinterpret_cast<const void*>(&conv_pw_frag_kernel<AFF, ACT>), lds);
    hipLaunchKernelGGL((conv_pw_frag_kernel<AFF, ACT>), grid, dim3(256), lds, stream, d, tilesN, M, d.C1, nk32, vec_out,
                       make_fastdiv(d.Ho * d.Wo));
}

// The instantiated prologue variants, X(mode, AFF, ACT): what the decoder / encoder 1x1 layers use.  The quick experiment builds
// (GA_PWF_EXP_ONLY) instantiate the first only.
#define GA_PWF_MODES_EXP(X) X(0x00, 0, GA_ACT_NONE)
#define GA_PWF_MODES(X)      \
    GA_PWF_MODES_EXP(X)      \
    X(0x01, 0, GA_ACT_SILU)  \
    X(0x10, 1, GA_ACT_NONE)  \
    X(0x11, 1, GA_ACT_SILU)  \
    X(0x20, 2, GA_ACT_NONE)

// GA_OK when tile code 12 takes the descriptor: the split-bf16 operands and vector output, 1x1 / stride 1 / pad 0, one source whose
// channel count is a multiple of the MFMA k step, whole 128-pixel tiles, no split-K, the fragment-ordered weight copy aligned when
// given, a prologue the decoder / encoder 1x1 layers use (a per-row affine needs the 16 pixels a staging thread converts to lie in
// one image)
int conv_pw_frag_check(const ga_conv_desc& d, const conv_req& r) {
    if (!(r.bf3 && r.vec_out)) return GA_E_UNSUPPORTED;
    if (d.KH != 1 || d.KW != 1 || d.sn != 1 || d.sd != 1 || d.pad != 0 || d.C2 != 0) return GA_E_UNSUPPORTED;
    if (d.Ho != d.Hi || d.Wo != d.Wi || d.C1 % 16 != 0 || r.splits != 1) return GA_E_UNSUPPORTED;
    if (((long)d.N * d.Ho * d.Wo) % 128 != 0) return GA_E_UNSUPPORTED;
    if (d.w_frag && !aligned16(d.w_frag)) return GA_E_UNSUPPORTED;
    const int mode = conv_pro_mode(d);
    switch (mode) {
        GA_PWF_MODES(GA_MODE_CASE) return mode != 0x20 || (d.Ho * d.Wo) % PSL == 0 ? GA_OK : GA_E_UNSUPPORTED;
        default: return GA_E_UNSUPPORTED;
    }
}

int conv_pw_frag_launch(const ga_conv_desc& d, const conv_req& r, hipStream_t stream) {
    constexpr int BM = 128, BN = 128;
    const int nk32 = (d.C1 + 31) / 32;
    const conv_tiling t = conv_tile_grid(d, BM, BN, 1, (size_t)2 * BM * PLD * 2);      // (whole tiles only: tilesM = M / 128)
#define GA_PWF(MODE, A, C) case MODE: launch_pw_frag_inst<A, C>(d, stream, t.grid, t.lds, t.tilesN, t.M, nk32, r.vec_out); break;
    switch (conv_pro_mode(d)) {
#ifdef GA_PWF_EXP_ONLY
        GA_PWF_MODES_EXP(GA_PWF)
#else
        GA_PWF_MODES(GA_PWF)
#endif
        default: return GA_E_UNSUPPORTED;
    }
#undef GA_PWF
    return check_launch();
}

}  // namespace ga

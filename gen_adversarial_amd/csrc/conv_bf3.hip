// conv_bf3 — the implicit-GEMM convolution of conv_mfma.hip on the bf16 matrix cores with fp32-class accuracy.
//
// On gfx950 the f32-input MFMA runs at the vector-ALU rate (64 FLOP/clk/SIMD); the bf16 MFMA runs 16x faster.  Every
// fp32 operand x is split as x = hi + lo + r with hi = bf16(x), lo = bf16(x - hi), |r| <= 2^-16 |x|, and
//     a*b  ~=  a_lo*b_hi + a_hi*b_lo + a_hi*b_hi        (three bf16 MFMAs, fp32 accumulation: mfma3 in conv_split.h)
// which keeps ~16 mantissa bits per product (relative error ~2e-5 per product, averaging down over K) — two orders
// of magnitude inside the path's 1e-3 parity bar — at 16/3 of the f32-MFMA rate.
//   * activations: split in registers by the loader, after the prologue (affine / SiLU / ELU / ReLU), right before
//     the LDS write: v_cvt_pk_bf16_f32 x2, shift back, subtract, v_cvt_pk again (12 VALU per float4; the bf16 matrix
//     pipe runs beside the VALU, unlike the f32 MFMA);
//   * weights: split once at load time on the host into two bf16 [Cout][K] arrays (w_hi, w_lo);
//   * LDS: four bf16 tiles per stage (A_hi, A_lo, B_hi, B_lo), rows of 32 k + 8 pad = 80 B: the 16-B fragment reads
//     of a 16-lane group fall on 16 distinct slots of the 256-B bank row (80*r mod 256 is a bijection on r < 16);
//   * fragments: lane (r = lane&31, h = lane>>5) reads the 8 bf16 A[r][8h..8h+7] / B[8h..8h+7][r] of a 16-deep k step
//     as ONE ds_read_b128 — exactly the operand layout of the 32x32x16 bf16 MFMA;
//   * everything else (gather by buffer loads with per-row offsets and tap masks, scalar K cursor, register
//     prefetch across the MFMAs, double-buffered LDS, LDS-transposed vector epilogue, split-K) is shared with the
//     fp32 kernel.  Shapes this kernel does not take (stride-2 transposes, channel counts not multiple of 8, the
//     3-channel image) run on the exact fp32-MFMA kernel.
#include "conv_split.h"
#include "conv_epilogue.h"
#include "conv_families.h"

namespace ga {

// -DGA_TRACE (make trace -> libga_ops_trace.so, tools/conv_trace.py): shader-clock stamps of the phases of each workgroup
#ifdef GA_TRACE
__device__ unsigned long long ga_trace_buf[8 * 8192];
#define GA_STAMP(i)                                                                                      \
    if (threadIdx.x == 0 && blockIdx.x < 8192 && blockIdx.y == 0) {                                      \
        ga_trace_buf[blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memtime();                              \
        if ((i) == 0) ga_trace_buf[blockIdx.x * 8 + 7] = __builtin_amdgcn_s_getreg((31 << 11) | 4);     \
    }
#else
#define GA_STAMP(i)
#endif

constexpr int BK3 = 32;     // k per LDS stage
constexpr int LDB = 40;     // bf16 elements per LDS row (32 + 8 pad = 80 B)

// AFF: 0 no affine, 1 per-channel scale/shift, 2 per-(row,channel) scale/shift.  ACT: the GA_ACT_* prologue activation.
// DUAL: a second K source (x2) exists (only without a prologue).  All three are compile-time so that the steady-state
// loop body is ONE basic block with no calls: the scheduler can then place the loader's VALU work (prologue + bf16
// split of tile t+1) BETWEEN the MFMAs of tile t (sched_group_barrier).  The lambdas are always_inline for the same
// reason — left to its heuristics the compiler outlined finish_tile in the larger instances, which put the staging
// registers in scratch and turned the LDS accesses into flat ones.
#ifndef GA_MINWG
#define GA_MINWG 2      // two workgroups per CU: the register budget is 256 per lane
#endif
template <int WM, int WN, int TM, int TN, int AFF, int ACT, bool DUAL>
__global__ void __launch_bounds__(256, GA_MINWG)
conv_bf3_kernel(const ga_conv_desc d, const int tilesN, const int M, const int Ctot, const int Ktot, const int nkc,
                const int vec_out, const fastdiv fd_howo, const fastdiv fd_wo) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    constexpr int RA = BM / 32;
    constexpr int RB = BN >= 64 ? BN / 64 : 1;
    constexpr int STAGE = (2 * BM + 2 * BN) * LDB;          // bf16 elements per stage
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __bf16* lds = reinterpret_cast<__bf16*>(smem);

    GA_STAMP(0)
    const int bid = xcd_tile_id();
    const int m0 = (bid / tilesN) * BM;
    const int n0 = (bid % tilesN) * BN;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int c4 = tid & 7, r0 = tid >> 3;                  // A staging: 8 channel-quads x 32 rows
    const int k8 = tid & 3, rb0 = tid >> 2;                 // B staging: 4 k-octets x 64 rows

    const int HoWo = d.Ho * d.Wo;
    constexpr int INV = 0x7fffffff;
    int a_n[RA], baseA[RA], baseA2[RA], baseB[RB];
    unsigned maskA[RA];
    const __amdgpu_buffer_rsrc_t rsrcX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.x), 0, d.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrcX2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.C2 > 0 ? d.x2 : d.x), 0,
                                                                             d.C2 > 0 ? d.x2_bytes : d.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrcWh = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(d.w_hi), 0, d.w_bytes / 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrcWl = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(d.w_lo), 0, d.w_bytes / 2, 0x00020000);
#pragma unroll
    for (int i = 0; i < RA; ++i) {
        const int m = m0 + r0 + 32 * i;
        unsigned mk = 0;
        int n = -1, h0 = 0, w0 = 0;
        if (m < M) {
            n = fd_div(m, fd_howo);
            const int rem = m - n * HoWo, ho = fd_div(rem, fd_wo), wo = rem - ho * d.Wo;
            h0 = ho * d.sn - d.pad; w0 = wo * d.sn - d.pad;
            mk = tap_mask(h0, w0, d.Hi, d.Wi, d.KH, d.KW);
        }
        a_n[i] = n;
        maskA[i] = mk;
        const int pixb = (n * d.Hi + h0) * d.Wi + w0;
        baseA[i] = pixb * d.ldx * 4 + c4 * 16;
        baseA2[i] = pixb * d.ldx2 * 4 + c4 * 16;
    }
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int row = rb0 + 64 * i;
        const int co = n0 + row;
        baseB[i] = (row < BN && co < d.Cout) ? (co * Ktot + 8 * k8) * 2 : INV;
    }

    static_assert(!DUAL || (AFF == 0 && ACT == GA_ACT_NONE), "a dual-source conv has no prologue");
    // staging registers: NSET sets.  With two, the loads of tile t+2 are issued at the START of iteration t (into the set
    // iteration t-1 drained) and consumed in iteration t+1: a whole iteration of MFMAs hides the L2 latency.  The
    // per-row-affine variant keeps one set (its scale/shift staging would not fit 256 registers twice).
    constexpr int NSET = AFF == 2 ? 1 : 2;
    floatx4 ra[NSET][RA], rs[NSET][AFF == 2 ? RA : 1], rt[NSET][AFF == 2 ? RA : 1];
    uintx4 rbh[NSET][RB], rbl[NSET][RB];
    unsigned okmask[NSET] = {};

    int q_tap = 0, q_chunk = 0, q_kh = 0, q_kw = 0;
    auto seek_tile = [&](const int t) __attribute__((always_inline)) {
        q_tap = __builtin_amdgcn_readfirstlane(t / nkc);
        q_chunk = __builtin_amdgcn_readfirstlane(t - q_tap * nkc);
        q_kh = __builtin_amdgcn_readfirstlane(q_tap / d.KW);
        q_kw = q_tap - q_kh * d.KW;
    };

    auto issue_tile = [&](const int set) __attribute__((always_inline)) {
        const int tap = q_tap, c0 = q_chunk * BK3;
        const int kh = q_kh, kw = q_kw;
        if (++q_chunk == nkc) { q_chunk = 0; ++q_tap; if (++q_kw == d.KW) { q_kw = 0; ++q_kh; } }
        const int c = c0 + 4 * c4;
        okmask[set] = 0;
        const bool in_x = DUAL ? c0 < d.C1 : true;
        const int lim = (in_x ? d.C1 : Ctot) - c0;
        const bool cval = 4 * c4 < lim;
        const int delta = (kh * d.Wi + kw) * (in_x ? d.ldx : d.ldx2) * 4;
        const int soffA = (in_x ? c0 : c0 - d.C1) * 4;
        const unsigned bit = 1u << tap;
        if (!DUAL || in_x) {
#pragma unroll
            for (int i = 0; i < RA; ++i) {
                const bool valid = cval & ((maskA[i] & bit) != 0);
                const int off = valid ? baseA[i] + delta : INV;
                okmask[set] |= (valid ? 1u : 0u) << i;
                ra[set][i] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(rsrcX, off, soffA, 0));
            }
        } else {
#pragma unroll
            for (int i = 0; i < RA; ++i) {
                const bool valid = cval & ((maskA[i] & bit) != 0);
                const int off = valid ? baseA2[i] + delta : INV;
                okmask[set] |= (valid ? 1u : 0u) << i;
                ra[set][i] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(rsrcX2, off, soffA, 0));
            }
        }
        const int soffB = (tap * Ctot + c0) * 2;
        const bool bval = c0 + 8 * k8 < Ctot;
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int off = bval ? baseB[i] : INV;
            rbh[set][i] = __builtin_amdgcn_raw_buffer_load_b128(rsrcWh, off, soffB, 0);
            rbl[set][i] = __builtin_amdgcn_raw_buffer_load_b128(rsrcWl, off, soffB, 0);
        }
        if (AFF == 1) {
            const int pc = cval ? c : 0;
            rs[set][0] = *reinterpret_cast<const floatx4*>(d.pro_scale + pc);
            rt[set][0] = *reinterpret_cast<const floatx4*>(d.pro_shift + pc);
        } else if (AFF == 2) {
#pragma unroll
            for (int i = 0; i < RA; ++i) {
                const size_t po = ((okmask[set] >> i) & 1u) ? (size_t)a_n[i] * d.C1 + c : 0;
                rs[set][i] = *reinterpret_cast<const floatx4*>(d.pro_scale + po);
                rt[set][i] = *reinterpret_cast<const floatx4*>(d.pro_shift + po);
            }
        }
    };

    auto finish_tile = [&](const int set, const int buf) __attribute__((always_inline)) {
        __bf16* Ah = lds + buf * STAGE;
        __bf16* Al = Ah + BM * LDB;
        __bf16* Bh = Al + BM * LDB;
        __bf16* Bl = Bh + BN * LDB;
        const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            floatx4 v = ra[set][i];
            if (AFF == 2) v = v * rs[set][i] + rt[set][i];
            else if (AFF == 1) v = pro_affine4(v, rs[set][0], rt[set][0], d.flags & GA_CONV_PRO_PRELU);
            v = pro_act4<ACT>(v);
            if (AFF != 0) v = (okmask[set] >> i) & 1u ? v : zero;     // act(0) = 0 for all three: only a shift un-zeroes padding
            bf16x4 hi, lo;
            split4(v, hi, lo);
            const int o = (r0 + 32 * i) * LDB + 4 * c4;
            *reinterpret_cast<bf16x4*>(Ah + o) = hi;
            *reinterpret_cast<bf16x4*>(Al + o) = lo;
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int row = rb0 + 64 * i;
            if (BN >= 64 || row < BN) {
                *reinterpret_cast<uintx4*>(Bh + row * LDB + 8 * k8) = rbh[set][i];
                *reinterpret_cast<uintx4*>(Bl + row * LDB + 8 * k8) = rbl[set][i];
            }
        }
    };

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int T = d.KH * d.KW * nkc;
    const int splits = gridDim.y, split = blockIdx.y;
    const int tper = (T + splits - 1) / splits;
    const int t_begin = split * tper;
    const int t_end = min(T, t_begin + tper);

    const int lrow = lane & 31, lh = lane >> 5;
    GA_STAMP(1)
    if (t_begin < t_end) {
        seek_tile(t_begin);
        issue_tile(0);
        if (NSET == 2 && t_begin + 1 < t_end) issue_tile(1);
        finish_tile(0, 0);
    }
    __syncthreads();
    GA_STAMP(2)
    auto mma_tile = [&](const int buf) __attribute__((always_inline)) {
        const __bf16* Ah = lds + buf * STAGE + (wm * TM * 32 + lrow) * LDB + 8 * lh;
        const __bf16* Al = Ah + BM * LDB;
        const __bf16* Bh = lds + buf * STAGE + 2 * BM * LDB + (wn * TN * 32 + lrow) * LDB + 8 * lh;
        const __bf16* Bl = Bh + BN * LDB;
#pragma unroll
        for (int ks = 0; ks < BK3 / 16; ++ks) {
            bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                ah[i] = *reinterpret_cast<const bf16x8*>(Ah + i * 32 * LDB + ks * 16);
                al[i] = *reinterpret_cast<const bf16x8*>(Al + i * 32 * LDB + ks * 16);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                bh[j] = *reinterpret_cast<const bf16x8*>(Bh + j * 32 * LDB + ks * 16);
                bl[j] = *reinterpret_cast<const bf16x8*>(Bl + j * 32 * LDB + ks * 16);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) mfma3(acc[i][j], ah[i], al[i], bh[j], bl[j]);
        }
    };

    // steady state: a next tile exists -> no branch in the body; the staging math of tile t+1 is spread between the
    // MFMAs of tile t (1 MFMA : 4 VALU : 1 DS, the matrix pipe takes 32 cycles per MFMA, a VALU op 4-8)
    constexpr int NMFMA = TM * TN * 3 * (BK3 / 16);
    // VALU ops of one staged tile: per float4 ~12 for the split, 4 affine, 20 SiLU/ELU, 4 ReLU, 4 padding select
    constexpr int VOPS = RA * (12 + (AFF ? 8 : 0) + (ACT == GA_ACT_SILU || ACT == GA_ACT_ELU ? 20 : ACT == GA_ACT_RELU ? 4 : ACT == GA_ACT_LRELU ? 8 : 0)) + 8;
    constexpr int VPM = (VOPS + NMFMA - 1) / NMFMA;
#ifndef GA_EXP
#define GA_EXP 0        // trace builds only: bit 0 drops the split + LDS write, 1 the global loads, 2 the barrier, 3 the MFMAs
#endif
    // one K step: [issue tile t+2 into the drained set] ; MFMAs of LDS stage `buf` || split + LDS write of tile t+1
    // (registers of set `cons`) into the other stage ; barrier.  `cons`/`prod` are literals at every call site.
    auto step = [&](const int buf, const int cons, const int prod, const bool more2) __attribute__((always_inline)) {
        if (NSET == 2 && more2 && !(GA_EXP & 2)) issue_tile(prod);
        if (!(GA_EXP & 8)) mma_tile(buf);
        if (!(GA_EXP & 1)) finish_tile(cons, buf ^ 1);
#pragma unroll
        for (int k = 0; k < NMFMA; ++k) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, VPM, 0);    // VALU
            __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);      // DS write
        }
        if (NSET == 1 && more2 && !(GA_EXP & 2)) issue_tile(prod);
        if (!(GA_EXP & 4)) __syncthreads();
    };
    // iteration t: LDS stage (t - t_begin) & 1 holds tile t; with two register sets, set (t + 1 - t_begin) & 1 holds
    // tile t+1 and tile t+2 is loaded into set (t - t_begin) & 1; with one set, tile t+2 is loaded after the split.
    int t = t_begin;
    if (NSET == 1 && t + 1 < t_end) issue_tile(0);      // tile t_begin+1
    for (; t + 1 < t_end; t += 2) {
        step(0, NSET == 2 ? 1 : 0, 0, t + 2 < t_end);
        if (t + 2 >= t_end) break;
        step(1, 0, NSET == 2 ? 1 : 0, t + 3 < t_end);
    }
    const int buf = (t_end - 1 - t_begin) & 1;          // the last tile's stage
    if (t_begin < t_end) mma_tile(buf);
    __syncthreads();        // every wave is done reading the operand tiles before the epilogue reuses the LDS
    GA_STAMP(3)

    conv_epilogue<WM, WN, TM, TN>(d, acc, smem, m0, n0, M, vec_out, splits, split);
    GA_STAMP(4)
}

template <int WM, int WN, int TM, int TN, int AFF, int ACT, bool DUAL>
static void launch_bf3_inst(const ga_conv_desc& d, hipStream_t stream, dim3 grid, size_t lds, int tilesN, int M, int Ctot,
                            int Ktot, int nkc, int vec_out) {
    const fastdiv fd_howo = make_fastdiv(d.Ho * d.Wo), fd_wo = make_fastdiv(d.Wo);
    static dyn_lds_cache attr;
    (void)ensure_dyn_lds(attr, reinterpret_cast<const void*>(&conv_bf3_kernel<WM, WN, TM, TN, AFF, ACT, DUAL>), lds);
    hipLaunchKernelGGL((conv_bf3_kernel<WM, WN, TM, TN, AFF, ACT, DUAL>), grid, dim3(256), lds, stream, d, tilesN, M, Ctot, Ktot, nkc, vec_out,
                       fd_howo, fd_wo);
}

// The instantiated prologue variants, X(mode, AFF, ACT, DUAL): the combinations the purification / classifier plans contain.
// mode = (dual << 8) | conv_pro_mode
#define GA_BF3_MODES(X)              \
    X(0x000, 0, GA_ACT_NONE, false)  \
    X(0x100, 0, GA_ACT_NONE, true)   \
    X(0x001, 0, GA_ACT_SILU, false)  \
    X(0x002, 0, GA_ACT_ELU, false)   \
    X(0x003, 0, GA_ACT_RELU, false)  \
    X(0x004, 0, GA_ACT_LRELU, false) \
    X(0x010, 1, GA_ACT_NONE, false)  \
    X(0x011, 1, GA_ACT_SILU, false)  \
    X(0x020, 2, GA_ACT_NONE, false)  \
    X(0x021, 2, GA_ACT_SILU, false)
static inline int conv_bf3_mode(const ga_conv_desc& d) { return ((d.C2 > 0 ? 1 : 0) << 8) | conv_pro_mode(d); }

// 1 when conv_bf3 has a kernel for this descriptor's prologue: part of ga_conv2d's `bf3`, which every split-bf16 family requires
int conv_bf3_mode_ok(const ga_conv_desc& d) {
    switch (conv_bf3_mode(d)) {
        GA_BF3_MODES(GA_MODE_CASE) return 1;
        default: return 0;
    }
}

template <int WM, int WN, int TM, int TN>
static int launch_bf3(const ga_conv_desc& d, hipStream_t stream, int vec_out, int splits) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const int Ctot = d.C1 + d.C2;
    const int Ktot = d.KH * d.KW * Ctot;
    const int nkc = (Ctot + BK3 - 1) / BK3;
    const conv_tiling t = conv_tile_grid(d, BM, BN, splits, (size_t)2 * (2 * BM + 2 * BN) * LDB * 2);
#define GA_BF3(MODE, A, C, D) \
    case MODE: launch_bf3_inst<WM, WN, TM, TN, A, C, D>(d, stream, t.grid, t.lds, t.tilesN, t.M, Ctot, Ktot, nkc, vec_out); break;
    switch (conv_bf3_mode(d)) {
        GA_BF3_MODES(GA_BF3)
        default: return GA_E_UNSUPPORTED;
    }
#undef GA_BF3
    return check_launch();
}

// tile codes 1 - 4 on the split-bf16 operands; ga_conv2d runs the fp32 family's tile of the same code when this refuses
int conv_bf3_check(const ga_conv_desc&, const conv_req& r) { return r.bf3 && r.tile >= 1 && r.tile <= 4 ? GA_OK : GA_E_UNSUPPORTED; }

// (the quick experiment builds compile tile 1 only and refuse the others here, past check)
int conv_bf3_launch(const ga_conv_desc& d, const conv_req& r, hipStream_t stream) {
    const int tile = r.tile, vec_out = r.vec_out, splits = r.splits;
    switch (tile) {
        case 1: return launch_bf3<2, 2, 2, 2>(d, stream, vec_out, splits);
#ifdef GA_TRACE_TILE1_ONLY      // quick experiment builds
        default: return GA_E_UNSUPPORTED;
    }
    switch (tile) {
#endif
        case 2: return launch_bf3<4, 1, 1, 2>(d, stream, vec_out, splits);
        case 3: return launch_bf3<2, 2, 1, 1>(d, stream, vec_out, splits);
        case 4: return launch_bf3<4, 1, 1, 1>(d, stream, vec_out, splits);
        default: return GA_E_UNSUPPORTED;
    }
}

}  // namespace ga

#ifdef GA_TRACE
extern "C" int ga_debug_trace_read(unsigned long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(ga::ga_trace_buf), (size_t)n * 8) == hipSuccess ? GA_OK : GA_E_LAUNCH;
}
#endif

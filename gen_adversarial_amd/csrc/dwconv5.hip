// ga_dwconv5 — depthwise 5x5 (pad 2) with fused activation prologue / act' epilogue, NHWC.
//
// Two windowed kernels and one for 4 x 4 images.  All share the thread layout: 8 channel-quads (float4, 16 B/lane => a
// pixel's 32 channels are one 128-B line) x 32 work lanes, one block = NB images x one window x 32 channels, the window staged
// in LDS once with the prologue activation applied once per staged element, zero-filled outside the image.  Staging issues
// its global loads in groups of 4 before touching them.  The 32-channel block is the fastest-varying part of blockIdx, so
// adjacent workgroups touch adjacent 128-B lines of the same pixels.
//
// The windowed kernel is bound by work per output (LDS reads, FMAs, one SiLU per staged element), not by HBM: it costs 16 LDS
// reads of 16 B + 25 FMAs per output float4 and runs at ~2.2 ps per output element whether it moves 5 or 12 bytes per output
// (DESIGN.md section 3).
//
//   plain and pool2 (dwconv5_kernel<SW>): (TH+4) x (TW+4) halo window, taps in LDS ([25][32]); each thread produces a strip of
//       SW horizontally adjacent outputs, a kernel row costs SW+4 input reads + 5 weight reads for 5*SW FMAs.  pool2 (the
//       adjoint of up2) is the 2x2 sum of the window results of two strips.
//
//   up2 forward (dwconv5_up2_kernel): y = dw5(nearest_x2(act(x))) + bias.  Output (2i+a, 2j+b), tap (kh, kw) reads
//       full-resolution pixel (2i+a+kh-2, 2j+b+kw-2), i.e. source pixel (i-1 + ((a+kh) >> 1), j-1 + ((b+kw) >> 1)):
//           a = 0: kh {0,1} {2,3} {4} fall on source rows i-1, i, i+1;  a = 1: kh {0} {1,2} {3,4};  the same along kw with b.
//       One source pixel of zero padding equals the full-resolution pad of 2 (rows -2, -1 -> source row -1; H, H+1 -> H/2).
//       Only the source window + 1 is staged (6 x 10 source pixels for 8 x 16 outputs instead of 12 x 20, SiLU once per
//       source element instead of four times); a thread produces the 2 x 4 outputs of two adjacent source pixels from a
//       3 x 4 source window: per kernel row 5 weight reads + 2 x 4 input reads for 40 FMAs (8 LDS reads per output float4).
//       Every output keeps the literal form's 25 products and their order (kh outer, kw inner, accumulator from zero, bias
//       last), so the result is BITWISE what the replicated-image form gave: the whole-model parity tests compare attack
//       trajectories that amplify a last-bit change.  Summing the taps that meet on one source pixel first (four 3x3 filters,
//       9 FMAs per output) is exact in real arithmetic (tests/test_dwconv5_subpixel_cpu.py) but moves the last bits; it
//       measured 5 - 12 % faster than this form (0.82 against 0.86 ms on the 64 x 64 layer).
//
// The up2 kernel keeps a pixel's two 64-B halves in two LDS planes 64 B (mod 256) apart, with 64 B per pixel in each: work
// lanes two pixels apart then fall on different 64-B quarters of the 256-B bank row and ds_read_b128 is conflict-free (with
// 128 B per pixel the lanes of a 16-lane group meet on two quarters: 2-way).
#include "ga_common.h"

namespace ga {

constexpr int DW_CC = 32;   // channels per block

// epilogue of every windowed form: v * act'(u) with u = dact_x row n / arep (K cotangents per forward row), stored at
// offset po of output row n (row_out floats per row)
__device__ __forceinline__ floatx4 dw_dact(const ga_dwconv5_desc& d, floatx4 v, const floatx4 u) {
    if (d.dact_act == GA_ACT_SILU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float sg = fast_sigmoid(u[e]); v[e] *= sg * (1.0f + u[e] * (1.0f - sg)); }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= act_bwd_fast(u[e], d.dact_act);
    }
    return v;
}

__device__ __forceinline__ void dw_finish(const ga_dwconv5_desc& d, floatx4 v, const int n, const size_t po,
                                          const size_t row_out, const int arep) {
    if (d.dact_x) v = dw_dact(d, v, *reinterpret_cast<const floatx4*>(d.dact_x + (size_t)(n / arep) * row_out + po));
    *reinterpret_cast<floatx4*>(d.y + (size_t)n * row_out + po) = v;
}

template <int SW>
__global__ void __launch_bounds__(256, 4)     // 4 workgroups per CU: the kernel is latency/HBM-bound, occupancy matters
dwconv5_kernel(const ga_dwconv5_desc d, const int NB, const int TH, const int TW, const int tilesH, const int tilesW,
               const int nchunks) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, c4 = tid & 7, pl = tid >> 3;

    int b = blockIdx.x;
    const int chunk = b % nchunks; b /= nchunks;
    const int tw = b % tilesW; b /= tilesW;
    const int th = b % tilesH; b /= tilesH;
    const int n0 = b * NB;
    const int nb = min(NB, d.N - n0);
    const int h0 = th * TH, w0 = tw * TW;
    const int c = chunk * DW_CC + 4 * c4;
    const bool cok = c < d.C;

    const int HH = TH + 4, WW = TW + 4;
    float* wS = smem;                         // [25][32]
    float* tile = smem + 25 * DW_CC;          // [nb][HH][WW][32]

    const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
    if (tid < 200) {                          // 25 taps x 8 channel-quads
        const int t = tid >> 3;
        *reinterpret_cast<floatx4*>(wS + t * DW_CC + 4 * c4) =
            cok ? *reinterpret_cast<const floatx4*>(d.w + (size_t)t * d.C + c) : zero;
    }
    floatx4 bias = zero;
    if (cok && d.bias) bias = *reinterpret_cast<const floatx4*>(d.bias + c);

    // ---- stage halo window: loads in groups of 4, then activation + LDS write
    const int halo_px = nb * HH * WW;
    for (int p0 = pl; p0 < halo_px; p0 += 32 * 4) {
        floatx4 v[4];
        bool ok[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int p = p0 + 32 * k;
            const int ww = p % WW; const int q = p / WW;
            const int hh = q % HH; const int ni = q / HH;
            const int h = h0 + hh - 2, w = w0 + ww - 2;
            ok[k] = cok && p < halo_px && h >= 0 && h < d.H && w >= 0 && w < d.W;
            const size_t off = ok[k] ? (((size_t)(n0 + ni) * d.H + h) * d.W + w) * d.C + c : 0;
            v[k] = *reinterpret_cast<const floatx4*>(d.x + off);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int p = p0 + 32 * k;
            if (p < halo_px) {
                floatx4 o = v[k];
                if (d.pro_act == GA_ACT_SILU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = o[e] * fast_sigmoid(o[e]);
                } else if (d.pro_act) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = act_fwd_fast(o[e], d.pro_act);
                }
                *reinterpret_cast<floatx4*>(tile + (size_t)p * DW_CC + 4 * c4) = ok[k] ? o : zero;
            }
        }
    }
    __syncthreads();
    if (!cok) return;

    // SW adjacent window results of output row hh starting at column ws (tile coordinates)
    auto strip = [&](const int ni, const int hh, const int ws, floatx4 (&acc)[SW]) {
#pragma unroll
        for (int j = 0; j < SW; ++j) acc[j] = zero;
        const float* base = tile + ((size_t)(ni * HH + hh) * WW + ws) * DW_CC + 4 * c4;
#pragma unroll 1
        for (int kh = 0; kh < 5; ++kh) {
            floatx4 w5[5], in[SW + 4];
#pragma unroll
            for (int kw = 0; kw < 5; ++kw) w5[kw] = *reinterpret_cast<const floatx4*>(wS + (kh * 5 + kw) * DW_CC + 4 * c4);
#pragma unroll
            for (int j = 0; j < SW + 4; ++j) in[j] = *reinterpret_cast<const floatx4*>(base + (kh * WW + j) * DW_CC);
#pragma unroll
            for (int j = 0; j < SW; ++j)
#pragma unroll
                for (int kw = 0; kw < 5; ++kw) acc[j] += in[j + kw] * w5[kw];
        }
    };

    const size_t row_out = (size_t)(d.pool2 ? (d.H / 2) * (d.W / 2) : d.H * d.W) * d.C;
    const int arep = d.act_rep > 1 ? d.act_rep : 1;
    const int th_n = min(TH, d.H - h0), tw_n = min(TW, d.W - w0);
    if (!d.pool2) {
        const int spr = (tw_n + SW - 1) / SW;                            // strips per row
        const int nst = nb * th_n * spr;
        for (int s = pl; s < nst; s += 32) {
            const int sx = s % spr; const int q = s / spr;
            const int hh = q % th_n; const int ni = q / th_n;
            floatx4 acc[SW];
            strip(ni, hh, sx * SW, acc);
#pragma unroll
            for (int j = 0; j < SW; ++j) {
                const int ww = sx * SW + j;
                if (ww < tw_n)
                    dw_finish(d, acc[j] + bias, n0 + ni, ((size_t)(h0 + hh) * d.W + (w0 + ww)) * d.C + c, row_out, arep);
            }
        }
    } else {
        // outputs at half resolution: SW must be even; a strip pair (rows 2r, 2r+1) yields SW/2 outputs
        const int Wo = d.W / 2;
        const int spr = (tw_n + SW - 1) / SW;
        const int nst = nb * (th_n / 2) * spr;
        for (int s = pl; s < nst; s += 32) {
            const int sx = s % spr; const int q = s / spr;
            const int hr = q % (th_n / 2); const int ni = q / (th_n / 2);
            floatx4 a0[SW], a1[SW];
            strip(ni, 2 * hr, sx * SW, a0);
            strip(ni, 2 * hr + 1, sx * SW, a1);
#pragma unroll
            for (int j = 0; j < SW; j += 2) {
                const int ww = sx * SW + j;
                if (ww < tw_n) {
                    const floatx4 v = a0[j] + a0[j + (SW > 1 ? 1 : 0)] + a1[j] + a1[j + (SW > 1 ? 1 : 0)];
                    dw_finish(d, v + bias, n0 + ni, ((size_t)(h0 / 2 + hr) * Wo + (w0 + ww) / 2) * d.C + c, row_out, arep);
                }
            }
        }
    }
}

// ---- up2 forward (header comment).  LDS: taps [25][32], then the window as two planes of 64 B per pixel
//      (channel quads 0-3 / 4-7), `plane` floats apart with plane * 4 = 64 (mod 256).

// stage nb windows of HH x WW pixels whose top-left is pixel (hb, wb) of the Hi x Wi images at d.x, zero outside the image,
// the prologue activation applied once per element; tq = this thread's quad of pixel 0 in its plane
__device__ __forceinline__ void dw_stage_split(const ga_dwconv5_desc& d, float* tq, const int n0, const int nb, const int HH,
                                               const int WW, const int hb, const int wb, const int Hi, const int Wi,
                                               const int c, const bool cok, const int pl) {
    const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
    const int npx = nb * HH * WW;
    for (int p0 = pl; p0 < npx; p0 += 32 * 8) {       // 8 loads in flight per thread: a 12 x 20 window is one round trip
        floatx4 v[8];
        bool ok[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int p = p0 + 32 * k;
            const int ww = p % WW; const int q = p / WW;
            const int hh = q % HH; const int ni = q / HH;
            const int h = hb + hh, w = wb + ww;
            ok[k] = cok && p < npx && h >= 0 && h < Hi && w >= 0 && w < Wi;
            const size_t off = ok[k] ? (((size_t)(n0 + ni) * Hi + h) * Wi + w) * d.C + c : 0;
            v[k] = *reinterpret_cast<const floatx4*>(d.x + off);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int p = p0 + 32 * k;
            if (p < npx) {
                floatx4 o = v[k];
                if (d.pro_act == GA_ACT_SILU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = o[e] * fast_sigmoid(o[e]);
                } else if (d.pro_act) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = act_fwd_fast(o[e], d.pro_act);
                }
                *reinterpret_cast<floatx4*>(tq + (size_t)p * 16) = ok[k] ? o : zero;
            }
        }
    }
}

// up2 forward.  TH x TW = the source tile (outputs 2TH x 2TW), window (TH+2) x WW with WW = TW rounded up to even + 2.
__global__ void __launch_bounds__(256, 4)
dwconv5_up2_kernel(const ga_dwconv5_desc d, const int NB, const int TH, const int TW, const int WW, const int plane,
                   const int tilesH, const int tilesW, const int nchunks) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, c4 = tid & 7, pl = tid >> 3;

    int b = blockIdx.x;
    const int chunk = b % nchunks; b /= nchunks;
    const int tw = b % tilesW; b /= tilesW;
    const int th = b % tilesH; b /= tilesH;
    const int n0 = b * NB;
    const int nb = min(NB, d.N - n0);
    const int Hs = d.H / 2, Ws = d.W / 2;
    const int h0 = th * TH, w0 = tw * TW;     // source coordinates
    const int c = chunk * DW_CC + 4 * c4;
    const bool cok = c < d.C;
    const int HH = TH + 2;
    float* wS = smem;                                                     // [25][32]
    float* tq = smem + 25 * DW_CC + (c4 >> 2) * plane + 4 * (c4 & 3);

    const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
    if (tid < 200) {                                                      // 25 taps x 8 channel-quads
        const int t = tid >> 3;
        *reinterpret_cast<floatx4*>(wS + t * DW_CC + 4 * c4) =
            cok ? *reinterpret_cast<const floatx4*>(d.w + (size_t)t * d.C + c) : zero;
    }
    floatx4 bias = zero;
    if (cok && d.bias) bias = *reinterpret_cast<const floatx4*>(d.bias + c);
    dw_stage_split(d, tq, n0, nb, HH, WW, h0 - 1, w0 - 1, Hs, Ws, c, cok, pl);
    __syncthreads();
    if (!cok) return;

    const size_t row_out = (size_t)d.H * d.W * d.C;
    const int arep = d.act_rep > 1 ? d.act_rep : 1;
    const int th_n = min(TH, Hs - h0), tw_n = min(TW, Ws - w0);
    const int spr = (tw_n + 1) / 2;                                       // pairs of source pixels per row
    const int nst = nb * th_n * spr;
    for (int it = pl; it < nst; it += 32) {
        const int sx = it % spr; const int q = it / spr;
        const int i = q % th_n; const int ni = q / th_n;
        floatx4 acc[2][4];                                                // [a][2 * j + b], j = source pixel of the pair, (a, b) = output parity
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[a][k] = zero;
        const float* base = tq + ((size_t)(ni * HH + i) * WW + 2 * sx) * 16;     // source pixel (i - 1, 2 sx - 1)
#pragma unroll 1
        for (int kh = 0; kh < 5; ++kh) {
            floatx4 w5[5];
#pragma unroll
            for (int kw = 0; kw < 5; ++kw) w5[kw] = *reinterpret_cast<const floatx4*>(wS + (kh * 5 + kw) * DW_CC + 4 * c4);
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                floatx4 in[4];                                            // window row (a + kh) >> 1
#pragma unroll
                for (int k = 0; k < 4; ++k) in[k] = *reinterpret_cast<const floatx4*>(base + (((a + kh) >> 1) * WW + k) * 16);
#pragma unroll
                for (int k = 0; k < 4; ++k)                               // output column 2 j + b of the pair, j = k >> 1, b = k & 1
#pragma unroll
                    for (int kw = 0; kw < 5; ++kw) acc[a][k] += in[(k >> 1) + (((k & 1) + kw) >> 1)] * w5[kw];
            }
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (2 * sx + (k >> 1) < tw_n)
                    dw_finish(d, acc[a][k] + bias, n0 + ni,
                              ((size_t)(2 * (h0 + i) + a) * d.W + (2 * (w0 + 2 * sx) + k)) * d.C + c, row_out, arep);
    }
}

// 4 x 4 images (the deepest decoder cells: 512 rows x 3072 channels = 12288 workgroups of 16 KB each in the windowed form, 88 us
// of mostly workgroup turnover): no halo frame — 16 images x 16 pixels x 32 channels in 32 KB of LDS, the border handled by
// the loop bounds (a 4 x 4 image meets 9 - 16 of the 25 taps per output, the others are skipped, not multiplied by zero).
// Work item = (image, output row, channel quad): four outputs from at most four input rows.
__global__ void __launch_bounds__(256, 4) dwconv5_4x4_kernel(const ga_dwconv5_desc d, const int nchunks) {
    constexpr int NB = 16;
    __shared__ __attribute__((aligned(16))) float wS[25 * DW_CC];
    __shared__ __attribute__((aligned(16))) float tile[NB * 16 * DW_CC];
    const int tid = threadIdx.x, c4 = tid & 7, pl = tid >> 3;
    const int chunk = blockIdx.x % nchunks;
    const int n0 = (blockIdx.x / nchunks) * NB;
    const int nb = min(NB, d.N - n0);
    const int c = chunk * DW_CC + 4 * c4;
    const bool cok = c < d.C;
    const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
    if (tid < 200) {
        const int t = tid >> 3;
        *reinterpret_cast<floatx4*>(wS + t * DW_CC + 4 * c4) = cok ? *reinterpret_cast<const floatx4*>(d.w + (size_t)t * d.C + c) : zero;
    }
    floatx4 bias = zero;
    if (cok && d.bias) bias = *reinterpret_cast<const floatx4*>(d.bias + c);
    // ---- stage nb * 16 pixels: 8 loads per thread, all issued before the first use
    {
        floatx4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int p = pl + 32 * k;
            const bool ok = cok && p < nb * 16;
            v[k] = ok ? *reinterpret_cast<const floatx4*>(d.x + ((size_t)n0 * 16 + p) * d.C + c) : zero;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int p = pl + 32 * k;
            floatx4 o = v[k];
            if (d.pro_act == GA_ACT_SILU) {
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = o[e] * fast_sigmoid(o[e]);
            } else if (d.pro_act) {
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = act_fwd_fast(o[e], d.pro_act);
            }
            *reinterpret_cast<floatx4*>(tile + p * DW_CC + 4 * c4) = o;
        }
    }
    __syncthreads();
    if (!cok) return;
    for (int s = pl; s < nb * 4; s += 32) {
        const int ni = s >> 2, h = s & 3;
        floatx4 acc[4] = {bias, bias, bias, bias};
        const int kh0 = max(0, 2 - h), kh1 = min(5, 6 - h);          // input row h + kh - 2 inside [0, 4)
        for (int kh = kh0; kh < kh1; ++kh) {
            const float* row = tile + ((ni * 4 + h + kh - 2) * 4) * DW_CC + 4 * c4;
            floatx4 in[4], w5[5];
#pragma unroll
            for (int j = 0; j < 4; ++j) in[j] = *reinterpret_cast<const floatx4*>(row + j * DW_CC);
#pragma unroll
            for (int kw = 0; kw < 5; ++kw) w5[kw] = *reinterpret_cast<const floatx4*>(wS + (kh * 5 + kw) * DW_CC + 4 * c4);
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int kw = j - w + 2;                       // compile-time after unrolling
                    if (kw >= 0 && kw < 5) acc[w] += in[j] * w5[kw];
                }
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const size_t o = (((size_t)(n0 + ni) * 4 + h) * 4 + w) * d.C + c;
            floatx4 v = acc[w];
            if (d.dact_x) {
                const int na = d.act_rep > 1 ? (n0 + ni) / d.act_rep : n0 + ni;       // K cotangents per forward row
                const floatx4 u = *reinterpret_cast<const floatx4*>(d.dact_x + (((size_t)na * 4 + h) * 4 + w) * d.C + c);
                if (d.dact_act == GA_ACT_SILU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const float sg = fast_sigmoid(u[e]); v[e] *= sg * (1.0f + u[e] * (1.0f - sg)); }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] *= act_bwd_fast(u[e], d.dact_act);
                }
            }
            *reinterpret_cast<floatx4*>(d.y + o) = v;
        }
    }
}

}  // namespace ga

extern "C" int ga_dwconv5(const ga_dwconv5_desc* dp, void* stream_) {
    ga::clear_stale_error();
    using namespace ga;
    if (!dp) return GA_E_BADARG;
    const ga_dwconv5_desc& d = *dp;
    if (!d.x || !d.w || !d.y || d.N <= 0 || d.H <= 0 || d.W <= 0 || d.C <= 0) return GA_E_BADARG;
    if (d.C % 4) return GA_E_UNSUPPORTED;
    if ((d.up2 || d.pool2) && ((d.H | d.W) & 1)) return GA_E_BADARG;
    if (d.up2 && d.pool2) return GA_E_UNSUPPORTED;
    if (d.act_rep > 1 && d.N % d.act_rep) return GA_E_BADARG;
    if (!aligned16(d.x) || !aligned16(d.w) || !aligned16(d.y) || (d.bias && !aligned16(d.bias)) ||
        (d.dact_x && !aligned16(d.dact_x))) return GA_E_ALIGN;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);

    const int nchunks = (d.C + DW_CC - 1) / DW_CC;
    if (d.H == 4 && d.W == 4 && !d.up2 && !d.pool2) {
        const long blocks = (((long)d.N + 15) / 16) * nchunks;                 // N + 15 in 64 bits: N may be INT_MAX
        if (blocks > 0x7fffffffL) return GA_E_UNSUPPORTED;
        hipLaunchKernelGGL(dwconv5_4x4_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d, nchunks);
        return check_launch();
    }
    if (d.up2) {
        // 8 x 16 source tiles (16 x 32 outputs): window 10 x 18 x 128 B = 22.5 KB, 64 work items of 2 x 4 outputs;
        // small images: several per workgroup, up to 64 work items in whole passes of the 32 lanes, inside 32 KB of LDS
        const int Hs = d.H / 2, Ws = d.W / 2;
        const int TH = Hs < 8 ? Hs : 8, TW = Ws < 16 ? Ws : 16;
        const int HH = TH + 2, WW = ((TW + 1) & ~1) + 2;
        const int items = TH * ((TW + 1) / 2);
        int NB = 64 / items;
        const int fit = (32 * 1024 - 25 * DW_CC * 4 - 2 * 80 * 4) / (HH * WW * DW_CC * 4);
        if (NB > fit) NB = fit;
        const int per32 = 32 / items;                                   // images per full pass of the 32 work lanes
        if (per32 > 1 && NB > per32) NB -= NB % per32;
        if (NB > d.N) NB = d.N;
        if (NB < 1) NB = 1;
        const int plane = ((NB * HH * WW * 16 + 63) & ~63) + 16;        // floats: a multiple of 256 B plus 64 B
        const int tilesH = (Hs + TH - 1) / TH, tilesW = (Ws + TW - 1) / TW;
        const long blocks = (((long)d.N + NB - 1) / NB) * tilesH * tilesW * nchunks;
        if (blocks > 0x7fffffffL) return GA_E_UNSUPPORTED;
        const size_t lds = (size_t)(25 * DW_CC + 2 * plane) * 4;
        hipLaunchKernelGGL(dwconv5_up2_kernel, dim3((unsigned)blocks), dim3(256), lds, stream, d, NB, TH, TW, WW, plane, tilesH, tilesW, nchunks);
        return check_launch();
    }
    // 8 x 16 output windows: (12 x 20) x 32 ch halo = 30 KB of LDS -> 4 workgroups per CU
    const int TH = d.H < 8 ? d.H : 8, TW = d.W < 16 ? d.W : 16;
    const int halo_bytes = (TH + 4) * (TW + 4) * DW_CC * 4;
    int NB = 256 / (TH * TW);
    if (NB < 1) NB = 1;
    const int fit = (40 * 1024 - 25 * DW_CC * 4) / halo_bytes;        // 4 workgroups x 40 KB = the CU's 160 KB
    if (NB > fit) NB = fit;
    if (NB > d.N) NB = d.N;
    if (NB < 1) NB = 1;
    const int tilesH = (d.H + TH - 1) / TH, tilesW = (d.W + TW - 1) / TW;
    const long blocks = (((long)d.N + NB - 1) / NB) * tilesH * tilesW * nchunks;
    if (blocks > 0x7fffffffL) return GA_E_UNSUPPORTED;
    const size_t lds = (size_t)NB * halo_bytes + 25 * DW_CC * 4;
    // strips of 4 when every tile width is a multiple of 4 (the strip reads SW+4 columns: stays inside the halo),
    // else strips of 2 (pool2 needs an even strip), else single outputs
    // (small images: strips of 2 when strips of 4 would leave half of the 32 strip lanes without work)
    const bool w2 = (d.W % 2 == 0) && (TW % 2 == 0);
    const bool w4 = (d.W % 4 == 0) && (TW % 4 == 0) && !(w2 && NB * TH * (TW / 4) < 32);
    if (w4) hipLaunchKernelGGL(dwconv5_kernel<4>, dim3((unsigned)blocks), dim3(256), lds, stream, d, NB, TH, TW, tilesH, tilesW, nchunks);
    else if (w2) hipLaunchKernelGGL(dwconv5_kernel<2>, dim3((unsigned)blocks), dim3(256), lds, stream, d, NB, TH, TW, tilesH, tilesW, nchunks);
    else {
        if (d.pool2) return GA_E_UNSUPPORTED;
        hipLaunchKernelGGL(dwconv5_kernel<1>, dim3((unsigned)blocks), dim3(256), lds, stream, d, NB, TH, TW, tilesH, tilesW, nchunks);
    }
    return check_launch();
}

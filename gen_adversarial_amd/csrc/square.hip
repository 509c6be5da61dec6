// ga_square_linf / ga_square_l2: one proposal per image of Square Attack (gen_adversarial_amd/attacks/square.py).  Every image draws
// its own window positions, channel signs and bump orientation from the generator of philox.h at (seed, draw, tensor, image row), as
// integers, so the host restatement (gen_adversarial_amd/attacks/square_ref.py) picks the same pixels bit for bit.  The numbers are
// defined in include/ga_ops.h.
#include "ga_common.h"
#include "philox.h"

using namespace ga;

namespace {

struct sq_args {
    int C, H, W, s;
    unsigned k0, k1, draw, tensor;
    unsigned long row0;
    const unsigned* image_row;            // counter word 1 of every image, or NULL: row0 + b
};

struct sq_choice {
    int h1, w1, h2, w2;                   // top-left corners of window 1 and window 2
    unsigned signs;                       // bit ch set: +
    bool transposed;
};

// pos(word, n) = (word * n) >> 32
__device__ __forceinline__ int sq_pos(const unsigned word, const int n) { return (int)__umulhi(word, (unsigned)n); }

__device__ __forceinline__ sq_choice sq_draw(const sq_args& a, const unsigned long b, const bool second) {
    const unsigned row = a.image_row ? a.image_row[b] : (unsigned)(a.row0 + b);
    unsigned x[4];
    philox4x32_10(0u, row, a.tensor, a.draw, a.k0, a.k1, x);
    sq_choice c;
    c.h1 = sq_pos(x[0], a.H - a.s + 1); c.w1 = sq_pos(x[1], a.W - a.s + 1);
    c.signs = x[2]; c.transposed = x[3] & 1u;
    c.h2 = c.h1; c.w2 = c.w1;
    if (second) {
        philox4x32_10(1u, row, a.tensor, a.draw, a.k0, a.k1, x);
        c.h2 = sq_pos(x[0], a.H - a.s + 1); c.w2 = sq_pos(x[1], a.W - a.s + 1);
    }
    return c;
}

__device__ __forceinline__ float clampf(const float v, const float lo, const float hi) { return fminf(fmaxf(v, lo), hi); }

// Store-bound, like nes_perturb_kernel: a 1-D grid-stride loop over the (image, channel, row, VEC columns) items.  An item copies
// x_adv, and where its row crosses window 1 replaces the columns inside by clamp(x_orig +- eps).  VEC = 4: 16-byte accesses
// (W % 4 == 0, aligned pointers); VEC = 1: any W.
template <int VEC>
__global__ void __launch_bounds__(256) square_linf_kernel(const sq_args a, const float* __restrict__ xo, const float* __restrict__ xa,
                                                          float* __restrict__ y, const float eps, const float lo, const float hi,
                                                          const unsigned long total) {
    const unsigned wq = (unsigned)a.W / VEC, plane = (unsigned)a.H * wq, per = (unsigned)a.C * plane;        // per image: < 2^31 items
    const unsigned long step = (unsigned long)gridDim.x * 256;
    for (unsigned long n = (unsigned long)blockIdx.x * 256 + threadIdx.x; n < total; n += step) {
        unsigned long b;
        unsigned r;
        if (total <= 0xffffffffUL) { b = (unsigned)n / per; r = (unsigned)n - (unsigned)b * per; }
        else { b = n / per; r = (unsigned)(n - b * per); }
        const unsigned ch = r / plane, rem = r - ch * plane;
        const int h = (int)(rem / wq), w = (int)(rem - (unsigned)h * wq) * VEC;
        const sq_choice c = sq_draw(a, b, false);
        const unsigned long at = (b * per + r) * VEC;
        alignas(16) float v[VEC];
        if constexpr (VEC == 4) *reinterpret_cast<floatx4*>(v) = *reinterpret_cast<const floatx4*>(xa + at);
        else v[0] = xa[at];
        if (h >= c.h1 && h < c.h1 + a.s && w + VEC > c.w1 && w < c.w1 + a.s) {
            const float e = (c.signs >> ch) & 1u ? eps : -eps;
            alignas(16) float o[VEC];
            if constexpr (VEC == 4) *reinterpret_cast<floatx4*>(o) = *reinterpret_cast<const floatx4*>(xo + at);
            else o[0] = xo[at];
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                if (w + j >= c.w1 && w + j < c.w1 + a.s) {
                    const float t = o[j] + e;
                    v[j] = lo <= hi ? clampf(t, lo, hi) : t;
                }
        }
        if constexpr (VEC == 4) *reinterpret_cast<floatx4*>(y + at) = *reinterpret_cast<const floatx4*>(v);
        else y[at] = v[0];
    }
}

// the sum of v over the wave, in every lane: a + b and b + a have the same bits, so the butterfly leaves one value
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// the four waves' partials of one quantity, added in wave order
__device__ __forceinline__ float waves4(const float* p) { return ((p[0] + p[1]) + p[2]) + p[3]; }

constexpr int SQ_MAXC = 32;

// One workgroup per image (see ga_ops.h for the formulas).  Four passes, each a strided walk by the 256 threads:
//   1. the whole image: per channel the sums of d^2 over the union of the windows and over window 1, and over all channels the
//      sum outside the union;  2. window 1: the norm of new[ch] per channel;  3. window 1: the sum of (scale[ch] new[ch])^2;
//   4. the whole image: y.  Every sum = per-thread partial in index order, wave butterfly, waves in order: fixed whatever the grid.
// new[] is recomputed where it is needed (s * s * C values, a division each) rather than stored: no buffer that grows with s.
__global__ void __launch_bounds__(256) square_l2_kernel(const sq_args a, const float* __restrict__ xo_, const float* __restrict__ xa_,
                                                        float* __restrict__ y_, const float* __restrict__ eta, const float eps,
                                                        const float lo, const float hi) {
    __shared__ float part[SQ_MAXC][3][4];         // [ch][union | window 1 | new][wave]
    __shared__ float part_o[4], part_e[4];        // outside the union; the rewritten window 1
    const unsigned long b = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6;
    const bool lead = (tid & 63) == 0;
    const int C = a.C, H = a.H, W = a.W, s = a.s, HW = H * W, ss = s * s;
    const sq_choice c = sq_draw(a, b, true);
    const float* xo = xo_ + b * (unsigned long)(C * HW);
    const float* xa = xa_ + b * (unsigned long)(C * HW);
    float* y = y_ + b * (unsigned long)(C * HW);

    // ---- pass 1
    float out = 0.0f;
    for (int ch = 0; ch < C; ++ch) {
        float un = 0.0f, w1 = 0.0f;
        for (int p = tid; p < HW; p += 256) {
            const int h = p / W, w = p - h * W;
            const float d = xa[ch * HW + p] - xo[ch * HW + p];
            const bool in1 = h >= c.h1 && h < c.h1 + s && w >= c.w1 && w < c.w1 + s;
            const bool in2 = h >= c.h2 && h < c.h2 + s && w >= c.w2 && w < c.w2 + s;
            const float dd = d * d;
            if (in1) w1 += dd;
            if (in1 || in2) un += dd; else out += dd;
        }
        un = wave_sum(un); w1 = wave_sum(w1);
        if (lead) { part[ch][0][wave] = un; part[ch][1][wave] = w1; }
    }
    out = wave_sum(out);
    if (lead) part_o[wave] = out;
    __syncthreads();
    const float n_out = waves4(part_o);
    float n_img = n_out, n_1 = 0.0f;
    for (int ch = 0; ch < C; ++ch) { n_img += waves4(part[ch][0]); n_1 += waves4(part[ch][1]); }
    const float den1 = 1e-12f + sqrtf(n_1);
    const float spare = fmaxf(eps * eps - n_img, 0.0f) / (float)C;

    // new[ch, i, j] of window pixel q = i * s + j
    auto fresh = [&](const int ch, const int q) {
        const int i = q / s, j = q - i * s;
        const float e = eta[c.transposed ? j * s + i : q];
        const int p = (c.h1 + i) * W + c.w1 + j;
        const float d = xa[ch * HW + p] - xo[ch * HW + p];
        return ((c.signs >> ch) & 1u ? e : -e) + d / den1;
    };

    // ---- pass 2
    for (int ch = 0; ch < C; ++ch) {
        float nn = 0.0f;
        for (int q = tid; q < ss; q += 256) { const float v = fresh(ch, q); nn += v * v; }
        nn = wave_sum(nn);
        if (lead) part[ch][2][wave] = nn;
    }
    __syncthreads();
    auto scale_of = [&](const int ch) { return sqrtf(spare + waves4(part[ch][0])) / (1e-12f + sqrtf(waves4(part[ch][2]))); };

    // ---- pass 3
    float ew = 0.0f;
    for (int ch = 0; ch < C; ++ch) {
        const float sc = scale_of(ch);
        for (int q = tid; q < ss; q += 256) { const float v = sc * fresh(ch, q); ew += v * v; }
    }
    ew = wave_sum(ew);
    if (lead) part_e[wave] = ew;
    __syncthreads();
    const float f = eps / (1e-12f + sqrtf(n_out + waves4(part_e)));

    // ---- pass 4
    for (int ch = 0; ch < C; ++ch) {
        const float sc = scale_of(ch);
        for (int p = tid; p < HW; p += 256) {
            const int h = p / W, w = p - h * W;
            const float o = xo[ch * HW + p];
            float d;
            if (h >= c.h1 && h < c.h1 + s && w >= c.w1 && w < c.w1 + s) d = sc * fresh(ch, (h - c.h1) * s + (w - c.w1));
            else if (h >= c.h2 && h < c.h2 + s && w >= c.w2 && w < c.w2 + s) d = 0.0f;
            else d = xa[ch * HW + p] - o;
            const float t = o + d * f;
            y[ch * HW + p] = lo <= hi ? clampf(t, lo, hi) : t;
        }
    }
}

// the checks both entry points share; fills `a`
int square_check(sq_args& a, long images, int C, int H, int W, int s, unsigned long seed, unsigned draw, unsigned tensor, unsigned long row0,
                 const unsigned* image_row) {
    if (images <= 0 || C <= 0 || H <= 0 || W <= 0) return GA_E_BADARG;
    if (s < 1 || s > (H < W ? H : W)) return GA_E_BADARG;
    const unsigned long lim = 1UL << 32;
    // row0 + images <= 2^32; with image_row the rows live on the device and every 32-bit word is a row
    if ((unsigned long)images > lim || (!image_row && (row0 > lim || (unsigned long)images > lim - row0))) return GA_E_BADARG;
    if (C > SQ_MAXC) return GA_E_UNSUPPORTED;                              // one sign bit per channel
    if ((unsigned long)C * (unsigned long)H * (unsigned long)W >= (1UL << 31)) return GA_E_UNSUPPORTED;     // int pixel indices
    a.C = C; a.H = H; a.W = W; a.s = s;
    a.k0 = (unsigned)(seed & 0xffffffffUL); a.k1 = (unsigned)(seed >> 32);
    a.draw = draw; a.tensor = tensor; a.row0 = row0; a.image_row = image_row;
    return GA_OK;
}

}  // namespace

extern "C" int ga_square_linf(const float* x_orig, const float* x_adv, float* y, long images, int C, int H, int W, int s, unsigned long seed,
                              unsigned draw, unsigned tensor, unsigned long row0, const unsigned* image_row, float eps, float lo, float hi,
                              void* stream) {
    ga::clear_stale_error();
    if (!x_orig || !x_adv || !y) return GA_E_BADARG;
    sq_args a;
    if (const int rc = square_check(a, images, C, H, W, s, seed, draw, tensor, row0, image_row)) return rc;
    const bool vec = W % 4 == 0 && aligned16(x_orig) && aligned16(x_adv) && aligned16(y);
    const unsigned long total = (unsigned long)images * ((unsigned long)C * H * W / (vec ? 4 : 1));
    const unsigned long blocks = (total + 255) / 256;
    const dim3 grid((unsigned)(blocks < (1UL << 20) ? blocks : (1UL << 20)));
    if (vec) hipLaunchKernelGGL(square_linf_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, a, x_orig, x_adv, y, eps, lo, hi, total);
    else hipLaunchKernelGGL(square_linf_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, a, x_orig, x_adv, y, eps, lo, hi, total);
    return check_launch();
}

extern "C" int ga_square_l2(const float* x_orig, const float* x_adv, float* y, const float* eta, long images, int C, int H, int W, int s,
                            unsigned long seed, unsigned draw, unsigned tensor, unsigned long row0, const unsigned* image_row, float eps,
                            float lo, float hi, void* stream) {
    ga::clear_stale_error();
    if (!x_orig || !x_adv || !y || !eta) return GA_E_BADARG;
    sq_args a;
    if (const int rc = square_check(a, images, C, H, W, s, seed, draw, tensor, row0, image_row)) return rc;
    if (images > 0x7fffffffL) return GA_E_UNSUPPORTED;                     // one workgroup per image
    hipLaunchKernelGGL(square_l2_kernel, dim3((unsigned)images), dim3(256), 0, (hipStream_t)stream, a, x_orig, x_adv, y, eta, eps, lo, hi);
    return check_launch();
}

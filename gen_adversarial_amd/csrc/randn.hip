// ga_randn: the defenders' N(0,1) draws from a counter-based generator (Philox4x32-10 + Box-Muller).  The numbers are defined in
// include/ga_ops.h and restated on the CPU by gen_adversarial_amd/noise.py: element e of absolute row R of tensor `tensor` at draw
// `draw` under `seed` depends on (seed, draw, tensor, R, e) alone, never on the launch geometry.
// Store-bound: one thread per quad = one Philox call, four normals, one 16-byte store.
#include "ga_common.h"
#include "philox.h"

using namespace ga;

namespace {

struct randn_args {
    float* y; long rows; unsigned long quads;      // quads per row (inner / 4)
    unsigned k0, k1, draw, stream; unsigned long row0;
    float scale; int mode;
};

// quad q of row r: the four values of y[r, 4q .. 4q+3] (the generator itself: philox.h)
__device__ __forceinline__ floatx4 randn_quad(const randn_args& a, const unsigned long r, const unsigned long q) {
    unsigned x[4];
    philox4x32_10((unsigned)q, (unsigned)(a.row0 + r), a.stream, a.draw, a.k0, a.k1, x);
    floatx4 v;
    if (a.mode == 1) {
        v[0] = __uint_as_float(x[0]); v[1] = __uint_as_float(x[1]); v[2] = __uint_as_float(x[2]); v[3] = __uint_as_float(x[3]);
        return v;
    }
    v = box_muller_quad(x);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = a.scale * v[j];
    return v;
}

// 1-D grid-stride loop over all quads of the tensor (64-bit indices; the division is 32-bit whenever the tensor allows it)
__global__ void __launch_bounds__(256) randn_kernel(const randn_args a, const unsigned long total) {
    const unsigned long step = (unsigned long)gridDim.x * 256;
    for (unsigned long i = (unsigned long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        unsigned long r, q;
        if (total <= 0xffffffffUL) { r = (unsigned)i / (unsigned)a.quads; q = (unsigned)i - (unsigned)r * (unsigned)a.quads; }
        else { r = i / a.quads; q = i - r * a.quads; }
        *reinterpret_cast<floatx4*>(a.y + i * 4) = randn_quad(a, r, q);
    }
}

// with coef: workgroup b serves quads [256 blk, 256 blk + 256) of row r = b / nblk alone (no workgroup straddles rows), and leaves
// the sum of its squares in ws[r * nblk + blk]: per-thread sum, six __shfl_xor steps per wave, the four waves added in wave order
__global__ void __launch_bounds__(256) randn_sumsq_kernel(const randn_args a, const unsigned nblk, float* __restrict__ ws) {
    __shared__ float part[4];
    const unsigned long r = blockIdx.x / nblk;
    const unsigned blk = blockIdx.x - (unsigned)r * nblk;
    const unsigned long q = (unsigned long)blk * 256 + threadIdx.x;
    float acc = 0.0f;
    if (q < a.quads) {
        const floatx4 v = randn_quad(a, r, q);
        *reinterpret_cast<floatx4*>(a.y + (r * a.quads + q) * 4) = v;
        acc = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) ws[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

// one thread per row adds the row's partials in index order
__global__ void __launch_bounds__(256) randn_coef_kernel(const float* __restrict__ ws, float* __restrict__ coef, const long rows, const unsigned nblk,
                                                         const float coef_eps) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const float* p = ws + r * nblk;
    float acc = 0.0f;
    for (unsigned b = 0; b < nblk; ++b) acc += p[b];
    coef[r] = coef_eps / sqrtf(acc);
}

}  // namespace

extern "C" int ga_randn(float* y, long rows, long inner, unsigned long seed, unsigned draw, unsigned tensor, unsigned long row0, float scale,
                        int mode, float* coef, float coef_eps, float* ws, long ws_floats, void* s) {
    ga::clear_stale_error();
    if (!y || rows <= 0 || inner <= 0 || mode < 0 || mode > 1) return GA_E_BADARG;
    if (inner % 4) return GA_E_UNSUPPORTED;
    if (row0 > (1UL << 32) || (unsigned long)rows > (1UL << 32) - row0) return GA_E_BADARG;      // row0 + rows <= 2^32
    if (!aligned16(y)) return GA_E_ALIGN;
    randn_args a;
    a.y = y; a.rows = rows; a.quads = (unsigned long)inner / 4;
    a.k0 = (unsigned)(seed & 0xffffffffUL); a.k1 = (unsigned)(seed >> 32);
    a.draw = draw; a.stream = tensor; a.row0 = row0; a.scale = scale; a.mode = mode;
    if (a.quads > (1UL << 32)) return GA_E_UNSUPPORTED;                   // counter word 0 is the quad
    if (coef) {
        if (mode != 0 || !ws) return GA_E_BADARG;
        const unsigned long nblk = (a.quads + 255) / 256;
        const unsigned long blocks = (unsigned long)rows * nblk;
        if (ws_floats < 0 || (unsigned long)ws_floats < blocks) return GA_E_BADARG;
        if (blocks > 0x7fffffffUL) return GA_E_UNSUPPORTED;
        hipLaunchKernelGGL(randn_sumsq_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, a, (unsigned)nblk, ws);
        hipLaunchKernelGGL(randn_coef_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)s,
                           (const float*)ws, coef, rows, (unsigned)nblk, coef_eps);
        return check_launch();
    }
    const unsigned long total = (unsigned long)rows * a.quads;
    const unsigned long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(randn_kernel, dim3((unsigned)(blocks < (1UL << 20) ? blocks : (1UL << 20))), dim3(256), 0, (hipStream_t)s, a, total);
    return check_launch();
}

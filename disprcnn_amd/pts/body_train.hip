// body_train.hip -- the weight gradient of a 1x1 convolution (stride 1 or 2) as a GEMM over pixels (gfx950).
//
//   gw[co][ci] = sum over (n, y, x) of  b[n, co, y, x] * a[n, ci, s*y, s*x]          (torch: conv2d's weight gradient, kernel 1, stride s)
//
// a (the layer's input) and b (the gradient of its output) are blocked tensors float[N][CB][H + 2ph][W + 2pw][16]: a pixel's 16 channels
// of one channel block are one 64-byte line.  That is the operand layout of v_mfma_f32_16x16x4_f32 as it stands: 16 lanes read one
// pixel's line, the four lane groups four consecutive pixels, and one MFMA adds four pixels (K = 4) to a 16 (co) x 16 (ci) tile.  No LDS.
//
// Work split.  The flat pixel index p = (n * OH + y) * OW + x is cut into chunks of `chunk` pixels (the caller's constant; the bits of
// the result depend on it and on nothing else).  A wave owns a 32 (co) x 32 (ci) tile of gw -- 2 x 2 MFMA tiles, so each loaded operand
// feeds two MFMAs -- and one chunk: it sums the chunk in fp32 in pixel order and stores its partial tile to
// scratch[chunk][cout][cin].  A tile's second channel block that does not exist (cb odd) is skipped: no loads, no MFMAs.  Rows and
// columns of a last channel block beyond cout / cin never leave the registers.  The finishing launch adds the partials of one element in
// chunk order in fp64 and rounds once (the rule of pn2_mlp_bwd.hip).  No atomics: the same bits run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_pts.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Operand {
    const float* p;
    int64_t n_stride, cb_stride, h_stride, off0;      // floats; off0: the interior's first element inside a (unit, channel block)
};

// one wave = one workgroup: tile (tb, ta) of 32 x 32, chunk c
__global__ __launch_bounds__(64) void conv1x1_wgrad_kernel(Operand a, Operand b, int64_t P, int OH, int OW, int stride, int cin, int cout,
                                                           int chunk, int64_t n_chunks, int tiles_a, float* __restrict__ partial) {
    const int lane = threadIdx.x, ch = lane & 15, kq = lane >> 4;
    const int64_t c = (int64_t)blockIdx.x % n_chunks;
    const int tile = (int)((int64_t)blockIdx.x / n_chunks);
    const int tb = tile / tiles_a, ta = tile % tiles_a;
    const int cb_a = (cin + 15) >> 4, cb_b = (cout + 15) >> 4;
    const bool a1 = 2 * ta + 1 < cb_a, b1 = 2 * tb + 1 < cb_b;                  // wave-uniform: the tile's second channel blocks exist
    const float* pa = a.p + (int64_t)(2 * ta) * a.cb_stride + a.off0 + ch;
    const float* pb = b.p + (int64_t)(2 * tb) * b.cb_stride + b.off0 + ch;
    const int64_t p0 = c * chunk, p1 = p0 + chunk < P ? p0 + chunk : P;
    const int hw = OH * OW;
    f32x4 acc00 = {0.f, 0.f, 0.f, 0.f}, acc01 = acc00, acc10 = acc00, acc11 = acc00;      // acc[co block][ci block]
#pragma unroll 2
    for (int64_t q = p0; q < p1; q += 4) {                                       // every lane takes every step: a pixel past the end adds 0
        const int64_t p = q + kq;
        const bool in = p < p1;
        float va0 = 0.f, va1 = 0.f, vb0 = 0.f, vb1 = 0.f;
        if (in) {
            const int n = (int)(p / hw), r = (int)(p - (int64_t)n * hw);
            const int y = r / OW, x = r - y * OW;
            const float* qa = pa + n * a.n_stride + (int64_t)(y * stride) * a.h_stride + (int64_t)(x * stride) * 16;
            const float* qb = pb + n * b.n_stride + (int64_t)y * b.h_stride + (int64_t)x * 16;
            va0 = qa[0];
            vb0 = qb[0];
            if (a1) va1 = qa[a.cb_stride];
            if (b1) vb1 = qb[b.cb_stride];
        }
        acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(vb0, va0, acc00, 0, 0, 0);
        if (a1) acc01 = __builtin_amdgcn_mfma_f32_16x16x4f32(vb0, va1, acc01, 0, 0, 0);
        if (b1) acc10 = __builtin_amdgcn_mfma_f32_16x16x4f32(vb1, va0, acc10, 0, 0, 0);
        if (a1 && b1) acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(vb1, va1, acc11, 0, 0, 0);
    }
    // D: column (ci) = lane & 15, row (co) = 4 * (lane >> 4) + register
    float* out = partial + c * ((int64_t)cout * cin);
    const int ci0 = 32 * ta + ch, ci1 = ci0 + 16, co0 = 32 * tb + 4 * kq;
    for (int r = 0; r < 4; ++r) {
        const int co = co0 + r;
        if (co < cout) {
            if (ci0 < cin) out[(int64_t)co * cin + ci0] = acc00[r];
            if (ci1 < cin) out[(int64_t)co * cin + ci1] = acc01[r];
        }
        if (co + 16 < cout) {
            if (ci0 < cin) out[(int64_t)(co + 16) * cin + ci0] = acc10[r];
            if (ci1 < cin) out[(int64_t)(co + 16) * cin + ci1] = acc11[r];
        }
    }
}

__global__ __launch_bounds__(256) void conv1x1_wgrad_finish_kernel(const float* __restrict__ partial, int64_t n_chunks, int64_t elems,
                                                                   float* __restrict__ gw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= elems) return;
    double s = 0.0;
    for (int64_t c = 0; c < n_chunks; ++c) s += (double)partial[c * elems + i];
    gw[i] = (float)s;
}

}  // namespace

extern "C" int drc_conv1x1_wgrad_default_chunk(void) { return 512; }

extern "C" int64_t drc_conv1x1_wgrad_scratch_floats(int N, int OH, int OW, int cin, int cout, int chunk) {
    if (N < 0 || OH <= 0 || OW <= 0 || cin <= 0 || cout <= 0 || chunk <= 0) return -1;
    const int64_t P = (int64_t)N * OH * OW;
    return (P + chunk - 1) / chunk * cout * cin;
}

extern "C" int drc_conv1x1_wgrad_blocked(const float* a, int64_t a_n_stride, int64_t a_cb_stride, int64_t a_h_stride, int64_t a_off0,
                                         const float* b, int64_t b_n_stride, int64_t b_cb_stride, int64_t b_h_stride, int64_t b_off0,
                                         int N, int OH, int OW, int cin, int cout, int stride, int chunk, float* gw, float* scratch,
                                         int64_t scratch_floats, void* stream) {
    if (N < 0 || OH <= 0 || OW <= 0 || cin <= 0 || cout <= 0 || chunk <= 0 || (stride != 1 && stride != 2) || !gw) return -2;
    if (a_n_stride < 0 || a_cb_stride < 0 || a_h_stride < 16 || a_off0 < 0 || b_n_stride < 0 || b_cb_stride < 0 || b_h_stride < 16 ||
        b_off0 < 0 || (int64_t)OH * OW > INT32_MAX)
        return -2;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t elems = (int64_t)cout * cin;
    const int64_t P = (int64_t)N * OH * OW;
    if (P == 0) {                                                   // an empty batch has a zero gradient
        hipError_t e = hipMemsetAsync(gw, 0, (size_t)elems * sizeof(float), st);
        return e == hipSuccess ? 0 : (int)e;
    }
    if (!a || !b || !scratch) return -2;
    const int64_t n_chunks = (P + chunk - 1) / chunk;
    if (scratch_floats < n_chunks * elems) return -3;
    const int tiles_a = (cin + 31) / 32, tiles_b = (cout + 31) / 32;
    const int64_t blocks = n_chunks * tiles_a * tiles_b;
    if (blocks > INT32_MAX || (elems + 255) / 256 > INT32_MAX) return -4;
    Operand oa = {a, a_n_stride, a_cb_stride, a_h_stride, a_off0}, ob = {b, b_n_stride, b_cb_stride, b_h_stride, b_off0};
    hipLaunchKernelGGL(conv1x1_wgrad_kernel, dim3((unsigned)blocks), dim3(64), 0, st, oa, ob, P, OH, OW, stride, cin, cout, chunk, n_chunks,
                       tiles_a, scratch);
    hipLaunchKernelGGL(conv1x1_wgrad_finish_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, scratch, n_chunks, elems, gw);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

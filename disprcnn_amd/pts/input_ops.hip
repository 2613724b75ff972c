// input_ops.hip -- the stereo input pipeline (gfx950): decoded uint8 images -> the padded fp32 batch of an ImageList, and the resize / flip
// of every instance mask of a batch.
//
//   reference: data/transforms/transforms.py (Resize, RandomHorizontalFlip, ToTensor, Normalize), structures/image_list.py:to_image_list,
//              structures/segmentation_mask.py:BinaryMaskList.resize / .transpose
//
// The transformed batch depends on the sample only through gathers and a 256-entry table per channel, so the host uploads the bytes and
// the tables (disprcnn_amd/data/device_input.py builds them) and everything else happens here.
//
// drc_input_batch_fwd.  out[i][c][y][x] = lut[c][ src_i[ytab_i[y]][xtab_i[x]][chan[c]] ] inside (out_h_i, out_w_i), +0.0 in the padding.
//   The output is walked as ONE flat array of I*3*Hp*Wp floats in quads of four consecutive elements; a quad may straddle a row, a plane
//   or an image (Wp is odd in the shipped configs), so every element of a quad is decomposed on its own by carrying (x, y, c, i) forward.
//   Quads are cut so that whole quads start on a 16-byte boundary of `out` whatever its alignment: quad q covers the elements
//   [4q - lead, 4q - lead + 4) clipped to [0, n), lead = the elements missing in front of the first boundary.  A whole quad is one
//   16-byte store, a clipped one (the first and the last at most) goes element by element.  Every element is written exactly once.
//   Reads cannot leave the buffers whatever the tables hold: table positions, table entries and the final byte index are clamped.
//
// drc_mask_resize_flip_fwd.  Per job (one BinaryMaskList): [G,H,W] uint8 0/1 -> [G,oh,ow]; the taps and weights are those of
//   mask_resize.h:resize_axis (torch's bilinear, align_corners=False); a pixel is 1 iff every tap whose fp32 weight is non-zero is 1,
//   which is what truncating the blend gives in exact arithmetic.  No floating-point sum.  flip reads the resized column ow-1-x.  A lane
//   owns four consecutive bytes of one job's output, stored as one dword when the job's pointer allows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_pts.h"
#include "mask_resize.h"

namespace {

constexpr int kThreads = 256;
constexpr int kDescInts = 8;          // image descriptor: src_off, src_h, src_w, out_h, out_w, ytab_off, xtab_off, 0
constexpr int kMaskCols = 10;         // mask job: src, dst, G, H, W, oh, ow, flip, first quad, quads
constexpr int kMaxMaskJobs = 4096;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int64_t clampl(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct Pos { int x, y, c, i; };

__device__ __forceinline__ float image_value(const uint8_t* __restrict__ src, int64_t src_bytes, const int32_t* __restrict__ tables,
                                             int64_t table_ints, const float* __restrict__ lut, int chan0, int chan1, int chan2, Pos p) {
    const int32_t* d = tables + (int64_t)p.i * kDescInts;
    const int out_h = d[3], out_w = d[4];
    if (p.y >= out_h || p.x >= out_w) return 0.f;
    const int src_h = d[1], src_w = d[2];
    const int sy = clampi(tables[clampl((int64_t)d[5] + p.y, 0, table_ints - 1)], 0, src_h - 1);
    const int sx = clampi(tables[clampl((int64_t)d[6] + p.x, 0, table_ints - 1)], 0, src_w - 1);
    const int ch = p.c == 0 ? chan0 : (p.c == 1 ? chan1 : chan2);
    const int64_t b = clampl((int64_t)d[0] + ((int64_t)sy * src_w + sx) * 3 + ch, 0, src_bytes - 1);
    return lut[p.c * 256 + src[b]];
}

__global__ __launch_bounds__(kThreads) void input_batch_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                               const int32_t* __restrict__ tables, int64_t table_ints,
                                                               const float* __restrict__ lut, int chan0, int chan1, int chan2, int Hp, int Wp,
                                                               float* __restrict__ out, int64_t n, int lead, int64_t quads) {
    const int64_t plane = (int64_t)Hp * Wp;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < quads; q += (int64_t)gridDim.x * kThreads) {
        const int64_t e0 = 4 * q - lead;                       // may be negative for q = 0
        const int64_t first = e0 < 0 ? 0 : e0;
        const int64_t last = e0 + 4 < n ? e0 + 4 : n;          // exclusive
        Pos p;
        if (n <= 0x7fffffff) {                                 // wave-uniform: 32-bit divisions for every batch that fits
            const uint32_t f = (uint32_t)first, pl = (uint32_t)plane, w = (uint32_t)Wp;
            const uint32_t ic = f / pl, r = f - ic * pl;
            p.i = (int)(ic / 3u); p.c = (int)(ic - 3u * (uint32_t)p.i);
            p.y = (int)(r / w); p.x = (int)(r - (uint32_t)p.y * w);
        } else {
            const int64_t ic = first / plane, r = first - ic * plane;
            p.i = (int)(ic / 3); p.c = (int)(ic - 3 * (int64_t)p.i);
            p.y = (int)(r / Wp); p.x = (int)(r - (int64_t)p.y * Wp);
        }
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t e = e0 + j;
            if (e >= first && e < last) {
                v[j] = image_value(src, src_bytes, tables, table_ints, lut, chan0, chan1, chan2, p);
                if (++p.x == Wp) {
                    p.x = 0;
                    if (++p.y == Hp) {
                        p.y = 0;
                        if (++p.c == 3) { p.c = 0; ++p.i; }
                    }
                }
            }
        }
        if (last - first == 4) {
            *reinterpret_cast<float4*>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e0 + j >= first && e0 + j < last) out[e0 + j] = v[j];
        }
    }
}

// 1 iff every tap of the axis pair with a non-zero weight is set
__device__ __forceinline__ int mask_pixel(const uint8_t* __restrict__ m, int W, drc_mask::Axis ay, drc_mask::Axis ax) {
    const uint8_t* r0 = m + (int64_t)ay.i0 * W;
    const uint8_t* r1 = m + (int64_t)ay.i1 * W;
    const bool y0 = ay.l0 != 0.f, y1 = ay.l1 != 0.f, x0 = ax.l0 != 0.f, x1 = ax.l1 != 0.f;
    bool on = true;
    if (y0 && x0) on = on && r0[ax.i0] != 0;
    if (y0 && x1) on = on && r0[ax.i1] != 0;
    if (y1 && x0) on = on && r1[ax.i0] != 0;
    if (y1 && x1) on = on && r1[ax.i1] != 0;
    return on ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void mask_resize_flip_kernel(const int64_t* __restrict__ jobs, int n_jobs, int64_t quads) {
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < quads; q += (int64_t)gridDim.x * kThreads) {
        int j = 0;
        while (j + 1 < n_jobs && jobs[(int64_t)(j + 1) * kMaskCols + 8] <= q) ++j;     // few jobs: a walk over their first quads
        const int64_t* d = jobs + (int64_t)j * kMaskCols;
        const int64_t k = q - d[8];
        if (k < 0 || k >= d[9]) continue;
        const uint8_t* src = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(d[0]));
        uint8_t* dst = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(d[1]));
        const int G = (int)d[2], H = (int)d[3], W = (int)d[4], oh = (int)d[5], ow = (int)d[6];
        const bool flip = d[7] != 0;
        const int64_t n = (int64_t)G * oh * ow, plane = (int64_t)oh * ow;
        const int64_t e0 = 4 * k;
        const int cnt = (int)(n - e0 < 4 ? n - e0 : 4);
        int64_t g = e0 / plane, r = e0 - g * plane;
        int y = (int)(r / ow), x = (int)(r - (int64_t)y * ow);
        uint32_t word = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t < cnt) {
                const drc_mask::Axis ay = drc_mask::resize_axis(y, H, oh);
                const drc_mask::Axis ax = drc_mask::resize_axis(flip ? ow - 1 - x : x, W, ow);
                word |= (uint32_t)mask_pixel(src + g * (int64_t)H * W, W, ay, ax) << (8 * t);
                if (++x == ow) {
                    x = 0;
                    if (++y == oh) { y = 0; ++g; }
                }
            }
        }
        if (cnt == 4 && (d[1] & 3) == 0) {
            *reinterpret_cast<uint32_t*>(dst + e0) = word;
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < cnt) dst[e0 + t] = (uint8_t)(word >> (8 * t));
        }
    }
}

int blocks_for(int64_t quads, int max_blocks) {
    int64_t b = (quads + kThreads - 1) / kThreads;
    if (b > max_blocks) b = max_blocks;
    return (int)(b < 1 ? 1 : b);
}

}  // namespace

extern "C" int drc_input_default_max_blocks(void) { return 8192; }

extern "C" int drc_input_batch_fwd(const uint8_t* src, int64_t src_bytes, const int32_t* tables, int64_t table_ints, const float* lut,
                                   int chan0, int chan1, int chan2, int I, int Hp, int Wp, float* out, int max_blocks, void* stream) {
    if (I < 0 || Hp < 0 || Wp < 0 || max_blocks < 1) return -1;
    if (chan0 < 0 || chan0 > 2 || chan1 < 0 || chan1 > 2 || chan2 < 0 || chan2 > 2) return -1;
    const int64_t n = (int64_t)I * 3 * Hp * Wp;
    if (n == 0) return 0;
    if (!src || !tables || !lut || !out || src_bytes < 1 || table_ints < (int64_t)I * kDescInts) return -1;
    if ((int64_t)Hp * Wp > 0x7fffffff) return -2;
    if (reinterpret_cast<uintptr_t>(out) & 3) return -1;
    const int lead = (int)((reinterpret_cast<uintptr_t>(out) >> 2) & 3);     // elements of the quad that lie in front of `out`
    const int64_t quads = (n + lead + 3) / 4;
    hipLaunchKernelGGL(input_batch_kernel, dim3(blocks_for(quads, max_blocks)), dim3(kThreads), 0, (hipStream_t)stream, src, src_bytes, tables,
                       table_ints, lut, chan0, chan1, chan2, Hp, Wp, out, n, lead, quads);
    return (int)hipGetLastError();
}

extern "C" int drc_mask_job_cols(void) { return kMaskCols; }

extern "C" int drc_mask_resize_flip_fwd(const int64_t* jobs, int n_jobs, int64_t quads, int max_blocks, void* stream) {
    if (n_jobs < 0 || n_jobs > kMaxMaskJobs || quads < 0 || max_blocks < 1) return -1;
    if (n_jobs == 0 || quads == 0) return 0;
    if (!jobs) return -1;
    hipLaunchKernelGGL(mask_resize_flip_kernel, dim3(blocks_for(quads, max_blocks)), dim3(kThreads), 0, (hipStream_t)stream, jobs, n_jobs, quads);
    return (int)hipGetLastError();
}

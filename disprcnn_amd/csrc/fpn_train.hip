// fpn_train.hip -- the two memory-bound pieces of the FPN's backward (gfx950 / CDNA4) on the engine's 16-channel blocked layout
// float[N][CB][H + 2p][W + 2p][16], one f32x4 (a channel quad) per lane:
//
//   drc_bilinear_resize_blocked_bwd   the adjoint of drc_bilinear_resize_blocked (align_corners = 0, upscaling) in GATHER form: one thread
//       owns an input pixel x channel quad, walks the output rows and columns that can have read it, recomputes the forward's own fp32
//       fy / fx / y0 / y1 / ty / tx (bilinear_up_blocked_kernel in volume_ops.hip, clamped neighbour included) and adds a term only where
//       the forward read this pixel -- in ascending (oy, ox) order, corner order (y0,x0) (y0,x1) (y1,x0) (y1,x1), so no atomics and the same
//       bits run to run.  An optional second gradient on the half-resolution grid [(IH-1)/2+1][(IW-1)/2+1] is added at the even positions:
//       the adjoint of max_pool2d(1, 2, 0) (LastLevelMaxPool).  Only the interior of grad_x is written.
//   drc_channel_sums_blocked          per-channel sums over all units and interior pixels (the bias gradient of a convolution with no
//       activation behind it), in fp64 in a FIXED order: per-block partials, then a finishing launch that adds them in block order.
// All element indices are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kThreads = 256;
constexpr int kMaxParts = 1024;      // partial sums per channel the finishing launch walks at most

inline unsigned grid_for(int64_t work, int cap = 256 * 16) {
    int64_t b = (work + kThreads - 1) / kThreads;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (unsigned)b;
}

// the forward's source index of output position o (ATen area_pixel_compute_source_index, align_corners = False), in its fp32 arithmetic
__device__ __forceinline__ void src_of(int o, float s, int I, int& i0, int& i1, float& t) {
    const float f = fmaxf(s * (o + 0.5f) - 0.5f, 0.f);
    i0 = (int)f;
    i1 = i0 + (i0 < I - 1);
    t = f - i0;
}

__global__ __launch_bounds__(kThreads) void bilinear_resize_blocked_bwd_kernel(const float* __restrict__ gy, float* __restrict__ gx,
                                                                               const float* __restrict__ gs, int N, int CB, int IH, int IW,
                                                                               int px, int OH, int OW, int py, int ps, int accumulate) {
    const int64_t total = (int64_t)N * CB * IH * IW * 4;
    const int64_t iW = IW + 2 * px, iH = IH + 2 * px, oW = OW + 2 * py, oH = OH + 2 * py;
    const int SH = (IH - 1) / 2 + 1, SW = (IW - 1) / 2 + 1;
    const int64_t sW = SW + 2 * ps, sH = SH + 2 * ps;
    const float sy = (float)IH / (float)OH, sx = (float)IW / (float)OW;       // the forward's scales
    const float ry = (float)OH / (float)IH, rx = (float)OW / (float)IW;       // their inverses: only bound the candidate range
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        int64_t t = idx;
        const int q = (int)(t & 3); t >>= 2;
        const int ix = (int)(t % IW); t /= IW;
        const int iy = (int)(t % IH); t /= IH;
        const int cb = (int)(t % CB);
        const int n = (int)(t / CB);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (gy) {
            // rows whose y0 or y1 can be iy have max(sy * (oy + 0.5) - 0.5, 0) in (iy - 1, iy + 1): oy in ((iy - 0.5) * ry - 0.5, (iy + 1.5) * ry - 0.5),
            // widened by one on each side against the rounding of this estimate and clamped (the clamped ends of the forward fall inside)
            int oy0 = (int)floorf((iy - 0.5f) * ry - 0.5f) - 1, oy1 = (int)ceilf((iy + 1.5f) * ry - 0.5f) + 1;
            int ox0 = (int)floorf((ix - 0.5f) * rx - 0.5f) - 1, ox1 = (int)ceilf((ix + 1.5f) * rx - 0.5f) + 1;
            if (oy0 < 0) oy0 = 0;
            if (ox0 < 0) ox0 = 0;
            if (oy1 > OH - 1) oy1 = OH - 1;
            if (ox1 > OW - 1) ox1 = OW - 1;
            const float* gb = gy + (((int64_t)n * CB + cb) * oH) * oW * 16 + q * 4;
            for (int oy = oy0; oy <= oy1; ++oy) {
                int y0, y1;
                float ty;
                src_of(oy, sy, IH, y0, y1, ty);
                const bool r0 = y0 == iy, r1 = y1 == iy;
                if (!(r0 || r1)) continue;
                for (int ox = ox0; ox <= ox1; ++ox) {
                    int x0, x1;
                    float tx;
                    src_of(ox, sx, IW, x0, x1, tx);
                    const bool c0 = x0 == ix, c1 = x1 == ix;
                    if (!(c0 || c1)) continue;
                    const f32x4 g = *(const f32x4*)(gb + ((int64_t)(oy + py) * oW + (ox + py)) * 16);
                    // the forward: v = (1 - ty) * ((1 - tx) * v00 + tx * v01) + ty * ((1 - tx) * v10 + tx * v11)
                    if (r0 && c0) acc += ((1.f - ty) * (1.f - tx)) * g;
                    if (r0 && c1) acc += ((1.f - ty) * tx) * g;
                    if (r1 && c0) acc += (ty * (1.f - tx)) * g;
                    if (r1 && c1) acc += (ty * tx) * g;
                }
            }
        }
        if (gs && !((iy | ix) & 1))
            acc += *(const f32x4*)(gs + ((((int64_t)n * CB + cb) * sH + (iy / 2 + ps)) * sW + (ix / 2 + ps)) * 16 + q * 4);
        float* dst = gx + ((((int64_t)n * CB + cb) * iH + (iy + px)) * iW + (ix + px)) * 16 + q * 4;
        *(f32x4*)dst = accumulate ? *(const f32x4*)dst + acc : acc;
    }
}

// grid (channel blocks, row chunks); block (4 channel quads, 64 pixel lanes).  Chunk b owns the rows [b * rows_per_block, ...) of the
// units * H interior rows.  Per thread in pixel order, then the 64 pixel lanes in lane order through LDS: one partial per channel and chunk.
__global__ __launch_bounds__(kThreads) void channel_sums_blocked_kernel(const float* __restrict__ x, double* __restrict__ part, int units, int CB,
                                                                        int H, int W, int ph, int pw, int rows_per_block) {
    __shared__ double red[64][16];
    const int q = threadIdx.x & 3, pl = threadIdx.x >> 2;
    const int cb = blockIdx.x;
    const int Hp = H + 2 * ph, Wp = W + 2 * pw;
    const int64_t cb_stride = (int64_t)Hp * Wp * 16, n_stride = cb_stride * CB;
    const int64_t rows = (int64_t)units * H;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    int64_t r1 = r0 + rows_per_block;
    if (r1 > rows) r1 = rows;
    const int64_t p0 = r0 * W, p1 = r1 * W;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int64_t p = p0 + pl; p < p1; p += 64) {
        const int64_t row = p / W;
        const int w = (int)(p - row * W);
        const int64_t u = row / H;
        const int h = (int)(row - u * H);
        const f32x4 v = *(const f32x4*)(x + u * n_stride + cb * cb_stride + ((int64_t)(h + ph) * Wp + (w + pw)) * 16 + q * 4);
        a0 += (double)v.x; a1 += (double)v.y; a2 += (double)v.z; a3 += (double)v.w;
    }
    red[pl][q * 4 + 0] = a0; red[pl][q * 4 + 1] = a1; red[pl][q * 4 + 2] = a2; red[pl][q * 4 + 3] = a3;
    __syncthreads();
    if (threadIdx.x < 16) {
        double s = red[0][threadIdx.x];
        for (int j = 1; j < 64; ++j) s += red[j][threadIdx.x];
        part[((int64_t)blockIdx.y * CB + cb) * 16 + threadIdx.x] = s;
    }
}

// sums[c] = the partials of channel c in chunk order (fp64), rounded once to fp32
__global__ __launch_bounds__(kThreads) void channel_sums_finish_kernel(const double* __restrict__ part, int nparts, int C16, float* __restrict__ sums) {
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= C16) return;
    double s = 0.0;
    for (int b = 0; b < nparts; ++b) s += part[(int64_t)b * C16 + c];
    sums[c] = (float)s;
}

int rows_per_block_for(int64_t rows) {
    int64_t per = (rows + kMaxParts - 1) / kMaxParts;
    if (per < 8) per = 8;
    return (int)per;
}

}  // namespace

extern "C" {

int drc_bilinear_resize_blocked_bwd(const float* grad_y, float* grad_x, int N, int CB, int IH, int IW, int px, int OH, int OW, int py,
                                    int align_corners, int accumulate, const float* grad_sub, int ps, void* stream) {
    if (N < 0 || CB <= 0 || IH <= 0 || IW <= 0 || px < 0 || ps < 0) return -2;
    if (grad_y && (align_corners || OH < IH || OW < IW || py < 0)) return -2;      // the FPN's top-down path only: align_corners = False, upscaling
    if (!grad_y && !grad_sub) return -2;
    const int64_t total = (int64_t)N * CB * IH * IW * 4;
    if (total == 0) return 0;
    if (!grad_x) return -1;
    hipLaunchKernelGGL(bilinear_resize_blocked_bwd_kernel, dim3(grid_for(total)), dim3(kThreads), 0, (hipStream_t)stream, grad_y, grad_x, grad_sub,
                       N, CB, IH, IW, px, grad_y ? OH : 1, grad_y ? OW : 1, grad_y ? py : 0, ps, accumulate ? 1 : 0);
    return (int)hipGetLastError();
}

int64_t drc_channel_sums_blocked_scratch_doubles(int units, int C, int H) {
    if (units <= 0 || C <= 0 || H <= 0) return 0;
    const int64_t rows = (int64_t)units * H;
    const int per = rows_per_block_for(rows);
    return (rows + per - 1) / per * ((C + 15) / 16 * 16);
}

int drc_channel_sums_blocked(const float* x, int units, int C, int H, int W, int ph, int pw, float* sums, double* scratch,
                             int64_t scratch_doubles, void* stream) {
    if (units < 0 || C <= 0 || H <= 0 || W <= 0 || ph < 0 || pw < 0) return -2;
    if (!sums) return -1;
    hipStream_t s = (hipStream_t)stream;
    const int CB = (C + 15) / 16;
    if (units == 0) return (int)hipMemsetAsync(sums, 0, sizeof(float) * CB * 16, s);
    if (!x) return -1;
    const int64_t rows = (int64_t)units * H;
    const int per = rows_per_block_for(rows);
    const int nparts = (int)((rows + per - 1) / per);
    if (!scratch || scratch_doubles < (int64_t)nparts * CB * 16) return -2;
    hipLaunchKernelGGL(channel_sums_blocked_kernel, dim3(CB, nparts), dim3(kThreads), 0, s, x, scratch, units, CB, H, W, ph, pw, per);
    // sums holds CB * 16 entries; those past C sum the zero padding channels
    hipLaunchKernelGGL(channel_sums_finish_kernel, dim3((CB * 16 + kThreads - 1) / kThreads), dim3(kThreads), 0, s, (const double*)scratch, nparts,
                       CB * 16, sums);
    return (int)hipGetLastError();
}

}  // extern "C"

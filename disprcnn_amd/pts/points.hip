// points.hip -- instance point clouds of the 3D stage (gfx950): PointRCNN.process_input_eval + back_project, eval form.
//
//   reference: pointnet_module/point_rcnn/lib/net/point_rcnn.py:37-83 (back_project), :189-241 (process_input_eval);
//              structures/calib.py:103-122 (img_to_rect, depthmap_to_rect); utils/utils_3d.py:74-104 (rotate_pc_along_y);
//              roi_heads/mask_head/inference.py:119-150 (Masker paste).
//
// The reference allocates two full-size maps per ROI, back-projects all H*W pixels of each, filters z > 0 and draws with NumPy,
// with a host sync per box.  Here kernel A visits box pixels only: one workgroup per ROI, x-major tiles (the order of
// meshgrid(x, y)), a ballot + LDS scan compacts the flat image index of each kept pixel.  The host reads the counts once,
// builds the draw, and kernel B recomputes the chosen points (the same device function, so bit-identical to what A kept),
// rotates them and subtracts a fixed-order mean.
//
// The training form (process_input + back_project with fix_seed=False, point_rcnn.py:97-187) is the same two kernels with TRAIN set:
// depth without the lower clamp (pixels of negative depth fall to the z > 0 filter), and in kernel B the augmentation in the
// reference's order: clamp at max_depth, times `scale`, x negated when flipped, the rotation by the angle negated when flipped.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_pts.h"

namespace {

constexpr int kA = 1024;              // kernel A: 16 waves per ROI
constexpr int kAWaves = kA / 64;
constexpr int kB = 256;               // kernel B: 4 waves per ROI

struct RoiBox { int x1, y1, x2, y2, x1p, x2p, H, W; };
struct PasteBox { int bx0, by0, bw, bh; };

__device__ __forceinline__ RoiBox load_box(const int32_t* __restrict__ roi_i, int r) {
    const int32_t* p = roi_i + (int64_t)r * 8;
    return RoiBox{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]};
}

// clipped pixel range of the box: [xlo, xhi) x [ylo, yhi)
__device__ __forceinline__ int64_t box_area(const RoiBox& b, int& xlo, int& xhi, int& ylo, int& yhi) {
    xlo = max(b.x1, 0); xhi = min(b.x2, b.W); ylo = max(b.y1, 0); yhi = min(b.y2, b.H);
    if (xhi <= xlo || yhi <= ylo) { xhi = xlo; yhi = ylo; return 0; }
    return (int64_t)(xhi - xlo) * (yhi - ylo);
}

// DisparityMap(d).resize((max(x2-x1, x2p-x1p), y2-y1)).crop(...) + x1 - x1p at box pixel (y, x): upsample_bilinear2d
// (align_corners=True), values / S * dst_w (structures/disparity.py:39-62), fp32 as the reference on float tensors
__device__ __forceinline__ float roi_disparity(const float* __restrict__ d, int S, const RoiBox& b, int y, int x) {
    const int hr = b.y2 - b.y1;
    const int wl = b.x2 - b.x1, wr = b.x2p - b.x1p;
    const int wd = wl > wr ? wl : wr;
    const float sh = hr > 1 ? (float)(S - 1) / (float)(hr - 1) : 0.f;
    const float sw = wd > 1 ? (float)(S - 1) / (float)(wd - 1) : 0.f;
    const float fy = sh * (float)(y - b.y1), fx = sw * (float)(x - b.x1);
    int y0 = (int)fy, x0 = (int)fx;
    y0 = y0 < S - 1 ? y0 : S - 1;
    x0 = x0 < S - 1 ? x0 : S - 1;
    const int yp = y0 < S - 1 ? 1 : 0, xp = x0 < S - 1 ? 1 : 0;
    float ly = fy - (float)y0, lx = fx - (float)x0;
    ly = fminf(fmaxf(ly, 0.f), 1.f); lx = fminf(fmaxf(lx, 0.f), 1.f);
    const float* r0 = d + (int64_t)y0 * S + x0;
    const float* r1 = r0 + (int64_t)yp * S;
    const float top = (1.f - lx) * r0[0] + lx * r0[xp];
    const float bot = (1.f - lx) * r1[0] + lx * r1[xp];
    const float v = (1.f - ly) * top + ly * bot;
    return (v / (float)S * (float)wd + (float)b.x1) - (float)b.x1p;
}

// depth_roi = fuxb / (disp + 1e-6) (Tensor.__rtruediv__ = reciprocal * fuxb), clamp(min=1.0) keeping NaN (point_rcnn.py:218-219);
// TRAIN: process_input's depth (:132-133), which has no clamp
template <bool TRAIN>
__device__ __forceinline__ float roi_depth(const float* __restrict__ d, int S, const RoiBox& b, int y, int x, float fuxb) {
    const float z = (1.f / (roi_disparity(d, S, b, y, x) + 1e-6f)) * fuxb;
    if (TRAIN) return z;
    return z < 1.f ? 1.f : z;
}

// expand_boxes + .to(int32) of paste_mask_in_image: box grown by (M + 2*pad) / M about its centre, truncated toward zero
__device__ __forceinline__ PasteBox paste_box(const float* __restrict__ b, int M, int pad) {
    const float scale = (float)((double)(M + 2 * pad) / (double)M);
    float w_half = (b[2] - b[0]) * 0.5f, h_half = (b[3] - b[1]) * 0.5f;
    const float xc = (b[2] + b[0]) * 0.5f, yc = (b[3] + b[1]) * 0.5f;
    w_half *= scale; h_half *= scale;
    const int x0 = (int)(xc - w_half), x1 = (int)(xc + w_half), y0 = (int)(yc - h_half), y1 = (int)(yc + h_half);
    PasteBox q;
    q.bx0 = x0; q.by0 = y0;
    q.bw = max(x1 - x0 + 1, 1); q.bh = max(y1 - y0 + 1, 1);
    return q;
}

// Masker value at image pixel (Y, X): F.interpolate(padded mask, (bh, bw), bilinear, align_corners=False) > thresh inside the
// pasted window, 0 elsewhere
__device__ __forceinline__ int masker_at(const float* __restrict__ prob, int M, int pad, const PasteBox& q, int Y, int X, int H, int W,
                                         float thresh) {
    const int x_lo = max(q.bx0, 0), x_hi = min(q.bx0 + q.bw, W), y_lo = max(q.by0, 0), y_hi = min(q.by0 + q.bh, H);
    if (X < x_lo || X >= x_hi || Y < y_lo || Y >= y_hi) return 0;
    const int P = M + 2 * pad;
    const float sy = (float)P / (float)q.bh, sx = (float)P / (float)q.bw;
    float fy = sy * ((float)(Y - q.by0) + 0.5f) - 0.5f, fx = sx * ((float)(X - q.bx0) + 0.5f) - 0.5f;
    fy = fy < 0.f ? 0.f : fy; fx = fx < 0.f ? 0.f : fx;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < P - 1 ? 1 : 0), x1 = x0 + (x0 < P - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    auto at = [&](int yy, int xx) -> float {
        yy -= pad; xx -= pad;
        return (yy >= 0 && yy < M && xx >= 0 && xx < M) ? prob[yy * M + xx] : 0.f;
    };
    const float top = (1.f - lx) * at(y0, x0) + lx * at(y0, x1);
    const float bot = (1.f - lx) * at(y1, x0) + lx * at(y1, x1);
    return ((1.f - ly) * top + ly * bot) > thresh ? 1 : 0;
}

__device__ __forceinline__ int64_t roi_offset(const int32_t* __restrict__ roi_i, int r) {
    int64_t off = 0;
    for (int q = 0; q < r; ++q) {
        int a, b, c, d;
        off += box_area(load_box(roi_i, q), a, b, c, d);
    }
    return off;
}

template <bool TRAIN>
__global__ __launch_bounds__(kA) void instance_points_kernel(const float* __restrict__ disp, int S, const int32_t* __restrict__ roi_i,
                                                            const float* __restrict__ roi_f, const float* __restrict__ mask, int M, int pad,
                                                            float thresh, int R, int64_t* __restrict__ info, int32_t* __restrict__ ws,
                                                            int64_t ws_cap) {
    __shared__ int wave_tot[kAWaves];
    const int r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RoiBox b = load_box(roi_i, r);
    const float* bf = roi_f + (int64_t)r * 12;
    const float fuxb = bf[10];
    const float* d = disp + (int64_t)r * S * S;
    const float* prob = mask + (int64_t)r * M * M;
    const PasteBox q = paste_box(bf, M, pad);
    int xlo, xhi, ylo, yhi;
    const int64_t area = box_area(b, xlo, xhi, ylo, yhi);
    const int hh = yhi - ylo;
    const int64_t off = roi_offset(roi_i, r);
    int64_t total = off;
    for (int qq = r; qq < R; ++qq) {
        int a0, a1, a2, a3;
        total += box_area(load_box(roi_i, qq), a0, a1, a2, a3);
    }
    const bool write = total <= ws_cap;

    // back_project's rule (:37-43): multiply by the mask only when it is non-empty and the masked depth has a positive pixel.
    // Depth is >= 1 (or NaN) inside the box and 0 outside, so that is "the mask meets the box at a pixel of non-NaN depth"; in the
    // training form it is "a masked box pixel has positive depth".
    int hit = 0;
    for (int64_t t = tid; t < area && !hit; t += kA) {
        const int x = xlo + (int)(t / hh), y = ylo + (int)(t % hh);
        if (masker_at(prob, M, pad, q, y, x, b.H, b.W, thresh)) hit = roi_depth<TRAIN>(d, S, b, y, x, fuxb) > 0.f;
    }
    const int use_mask = __syncthreads_or(hit);

    int64_t run = 0;
    for (int64_t base = 0; base < area; base += kA) {
        const int64_t t = base + tid;
        int keep = 0, x = 0, y = 0;
        if (t < area) {
            x = xlo + (int)(t / hh); y = ylo + (int)(t % hh);
            float z = roi_depth<TRAIN>(d, S, b, y, x, fuxb);
            if (use_mask) z = z * (float)masker_at(prob, M, pad, q, y, x, b.H, b.W, thresh);
            keep = z > 0.f;
        }
        const uint64_t bal = __ballot(keep);
        const int below = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, tile = 0;
        for (int w = 0; w < kAWaves; ++w) {
            const int c = wave_tot[w];
            before += w < wave ? c : 0;
            tile += c;
        }
        if (keep && write) ws[off + run + before + below] = y * b.W + x;
        run += tile;
        __syncthreads();
    }
    if (tid == 0) {
        info[r] = run;
        info[R + r] = off;
        if (r == 0) info[2 * R] = total;
    }
}

template <bool TRAIN>
__global__ __launch_bounds__(kB) void instance_points_gather_kernel(const float* __restrict__ disp, int S, const int32_t* __restrict__ roi_i,
                                                                   const float* __restrict__ roi_f, const double* __restrict__ roi_d, int R,
                                                                   const int64_t* __restrict__ info, const int32_t* __restrict__ ws,
                                                                   const int32_t* __restrict__ choice, int npoints, float max_depth,
                                                                   float* __restrict__ pts, float* __restrict__ mean, double* __restrict__ rot,
                                                                   int32_t* __restrict__ src_pix, float scale, int flip) {
    __shared__ float red[3][kB];
    const int r = blockIdx.x, tid = threadIdx.x;
    const RoiBox b = load_box(roi_i, r);
    const float* bf = roi_f + (int64_t)r * 12;
    const float fu = bf[4], fv = bf[5], cu = bf[6], cv = bf[7], tx = bf[8], ty = bf[9], fuxb = bf[10], half_w0 = bf[11];
    const float* d = disp + (int64_t)r * S * S;
    const int64_t n = info[r], off = info[R + r];
    if (n <= 0) return;                             // the caller raises before launching on a ROI without a point
    // rotate_pc_along_y: centre in fp32 ((x1 + x2) / 2 - W/2), atan2 in fp64 against the fp64 focal length, cos/sin cast to fp32
    const float cw = (bf[0] + bf[2]) / 2.f - half_w0;
    double ang = atan2((double)cw, roi_d[r]);
    if (TRAIN && flip) ang = -ang;                  // rotator.rot_angle *= -1 (point_rcnn.py:161)
    const float c = (float)cos(ang), s = (float)sin(ang), ns = (float)(-sin(ang));
    float* out = pts + (int64_t)r * npoints * 3;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int i = tid; i < npoints; i += kB) {
        int j = choice[(int64_t)r * npoints + i];
        j = (j >= 0 && j < n) ? j : 0;
        const int p = ws[off + j];
        const int y = p / b.W, x = p - y * b.W;
        const float z = roi_depth<TRAIN>(d, S, b, y, x, fuxb);
        // img_to_rect (calib.py:103-110), then clamp(z, max=max_depth) (point_rcnn.py:81)
        float px = (((float)x - cu) * z) / fu + tx;
        float py = (((float)y - cv) * z) / fv + ty;
        float pz = z > max_depth ? max_depth : z;
        if (TRAIN) {                                // pts * scale, then x = -x (point_rcnn.py:145-156)
            px *= scale; py *= scale; pz *= scale;
            if (flip) px = -px;
        }
        // [x, z] @ [[c, -s], [s, c]]^T
        const float rx = px * c + pz * ns;
        const float rz = px * s + pz * c;
        out[i * 3 + 0] = rx; out[i * 3 + 1] = py; out[i * 3 + 2] = rz;
        sx += rx; sy += py; sz += rz;
        if (src_pix) src_pix[(int64_t)r * npoints + i] = p;
    }
    red[0][tid] = sx; red[1][tid] = sy; red[2][tid] = sz;
    __syncthreads();
    for (int h = kB / 2; h > 0; h >>= 1) {          // fixed pairing: the same sum order on every run
        if (tid < h) {
            red[0][tid] += red[0][tid + h]; red[1][tid] += red[1][tid + h]; red[2][tid] += red[2][tid + h];
        }
        __syncthreads();
    }
    const float mx = red[0][0] / (float)npoints, my = red[1][0] / (float)npoints, mz = red[2][0] / (float)npoints;
    for (int i = tid; i < npoints; i += kB) {
        out[i * 3 + 0] -= mx; out[i * 3 + 1] -= my; out[i * 3 + 2] -= mz;
    }
    if (tid == 0) {
        mean[r * 3 + 0] = mx; mean[r * 3 + 1] = my; mean[r * 3 + 2] = mz;
        rot[r] = ang;
    }
}

}  // namespace

extern "C" const char* drc_pts_version(void) { return "disprcnn_pts gfx950 1"; }

extern "C" int drc_instance_points_fwd(const float* disp, int S, const int32_t* roi_i, const float* roi_f, const float* mask, int M, int pad,
                                       float thresh, int R, int64_t* info, int32_t* ws, int64_t ws_cap, void* stream) {
    if (R < 0 || S <= 0 || M <= 0 || pad < 0 || ws_cap < 0) return -2;
    if (R == 0) return 0;
    if (!disp || !roi_i || !roi_f || !mask || !info || (ws_cap > 0 && !ws)) return -1;
    hipLaunchKernelGGL(instance_points_kernel<false>, dim3((unsigned)R), dim3(kA), 0, (hipStream_t)stream, disp, S, roi_i, roi_f, mask, M, pad,
                       thresh, R, info, ws, ws_cap);
    return (int)hipGetLastError();
}

extern "C" int drc_instance_points_train_fwd(const float* disp, int S, const int32_t* roi_i, const float* roi_f, const float* mask, int M, int pad,
                                             float thresh, int R, int64_t* info, int32_t* ws, int64_t ws_cap, void* stream) {
    if (R < 0 || S <= 0 || M <= 0 || pad < 0 || ws_cap < 0) return -2;
    if (R == 0) return 0;
    if (!disp || !roi_i || !roi_f || !mask || !info || (ws_cap > 0 && !ws)) return -1;
    hipLaunchKernelGGL(instance_points_kernel<true>, dim3((unsigned)R), dim3(kA), 0, (hipStream_t)stream, disp, S, roi_i, roi_f, mask, M, pad,
                       thresh, R, info, ws, ws_cap);
    return (int)hipGetLastError();
}

extern "C" int drc_instance_points_gather_fwd(const float* disp, int S, const int32_t* roi_i, const float* roi_f, const double* roi_d, int R,
                                              const int64_t* info, const int32_t* ws, const int32_t* choice, int npoints, float max_depth,
                                              float* pts, float* mean, double* rot, int32_t* src_pix, void* stream) {
    if (R < 0 || S <= 0 || npoints <= 0) return -2;
    if (R == 0) return 0;
    if (!disp || !roi_i || !roi_f || !roi_d || !info || !ws || !choice || !pts || !mean || !rot) return -1;
    hipLaunchKernelGGL(instance_points_gather_kernel<false>, dim3((unsigned)R), dim3(kB), 0, (hipStream_t)stream, disp, S, roi_i, roi_f, roi_d, R,
                       info, ws, choice, npoints, max_depth, pts, mean, rot, src_pix, 1.f, 0);
    return (int)hipGetLastError();
}

extern "C" int drc_instance_points_gather_train_fwd(const float* disp, int S, const int32_t* roi_i, const float* roi_f, const double* roi_d, int R,
                                                    const int64_t* info, const int32_t* ws, const int32_t* choice, int npoints, float max_depth,
                                                    float scale, int flip, float* pts, float* mean, double* rot, int32_t* src_pix, void* stream) {
    if (R < 0 || S <= 0 || npoints <= 0) return -2;
    if (R == 0) return 0;
    if (!disp || !roi_i || !roi_f || !roi_d || !info || !ws || !choice || !pts || !mean || !rot) return -1;
    hipLaunchKernelGGL(instance_points_gather_kernel<true>, dim3((unsigned)R), dim3(kB), 0, (hipStream_t)stream, disp, S, roi_i, roi_f, roi_d, R,
                       info, ws, choice, npoints, max_depth, pts, mean, rot, src_pix, scale, flip ? 1 : 0);
    return (int)hipGetLastError();
}

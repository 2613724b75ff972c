// box3d_iou.h -- the rotated-overlap device code that boxes3d.hip and proposal_target.hip share: a box's derived geometry (BoxG), the
// rotated BEV overlap (box_overlap) and the 3D IoU of boxes_iou3d_gpu after it, in its torch order.
//
//   reference: point_rcnn/lib/utils/iou3d/src/iou3d_kernel.cu (box_overlap and what it calls), iou3d_utils.py (boxes_iou3d_gpu),
//              utils/kitti_utils.py (boxes3d_to_bev_torch)
//
// Every value is the reference's fp32 expression in its order (the library builds with -ffp-contract=off).  box_overlap uses wave
// votes to cut its loops short: every lane of a wave must call it.
#ifndef DISPRCNN_BOX3D_IOU_H
#define DISPRCNN_BOX3D_IOU_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace box3d_iou {

constexpr float kEps = 1e-8f;               // iou3d_kernel.cu EPS
constexpr float kMargin = 1e-5f;            // check_in_box2d MARGIN
constexpr int kPoly = 24;                   // 16 edge intersections + 8 corners

// One box [x1, y1, x2, y2, ry], everything box_overlap / check_in_box2d / iou_bev derive from it alone.
struct BoxG {
    float x1, y1, x2, y2;
    float cx, cy;                           // (x1 + x2) / 2, (y1 + y2) / 2
    float cn, sn;                           // cos(-ry), sin(-ry): check_in_box2d
    float px[4], py[4];                     // corners (x1,y1) (x2,y1) (x2,y2) (x1,y2) rotated about the centre by ry
    float area;                             // (x2 - x1) * (y2 - y1): iou_bev
};

__device__ __forceinline__ BoxG box_geom(float x1, float y1, float x2, float y2, float ry) {
    BoxG g;
    g.x1 = x1; g.y1 = y1; g.x2 = x2; g.y2 = y2;
    g.cx = (x1 + x2) / 2;
    g.cy = (y1 + y2) / 2;
    g.cn = cosf(-ry);
    g.sn = sinf(-ry);
    const float c = cosf(ry), s = sinf(ry);
    const float xs[4] = {x1, x2, x2, x1}, ys[4] = {y1, y1, y2, y2};
#pragma unroll
    for (int k = 0; k < 4; ++k) {           // rotate_around_center
        g.px[k] = (xs[k] - g.cx) * c + (ys[k] - g.cy) * s + g.cx;
        g.py[k] = -(xs[k] - g.cx) * s + (ys[k] - g.cy) * c + g.cy;
    }
    g.area = (x2 - x1) * (y2 - y1);
    return g;
}

__device__ __forceinline__ BoxG box_geom5(const float* b) { return box_geom(b[0], b[1], b[2], b[3], b[4]); }

// kitti_utils.boxes3d_to_bev_torch of one [x, y, z, h, w, l, ry] box
__device__ __forceinline__ BoxG box_geom7(const float* b) {
    const float half_l = b[5] / 2, half_w = b[4] / 2;
    return box_geom(b[0] - half_l, b[2] - half_w, b[0] + half_l, b[2] + half_w, b[6]);
}

__device__ __forceinline__ bool in_box2d(const BoxG& g, float x, float y) {      // check_in_box2d
    const float rx = (x - g.cx) * g.cn + (y - g.cy) * g.sn + g.cx;
    const float ry = -(x - g.cx) * g.sn + (y - g.cy) * g.cn + g.cy;
    return rx > g.x1 - kMargin && rx < g.x2 + kMargin && ry > g.y1 - kMargin && ry < g.y2 + kMargin;
}

__device__ __forceinline__ float cross3(float p1x, float p1y, float p2x, float p2y, float p0x, float p0y) {
    return (p1x - p0x) * (p2y - p0y) - (p2x - p0x) * (p1y - p0y);
}

// intersection(p1, p0, q1, q0, ans): segment p0-p1 against q0-q1
__device__ __forceinline__ bool intersection(float p1x, float p1y, float p0x, float p0y, float q1x, float q1y, float q0x, float q0y,
                                             float& ax, float& ay) {
    const bool rect = fminf(p0x, p1x) <= fmaxf(q0x, q1x) && fminf(q0x, q1x) <= fmaxf(p0x, p1x) &&
                      fminf(p0y, p1y) <= fmaxf(q0y, q1y) && fminf(q0y, q1y) <= fmaxf(p0y, p1y);
    if (!rect) return false;
    const float s1 = cross3(q0x, q0y, p1x, p1y, p0x, p0y);
    const float s2 = cross3(p1x, p1y, q1x, q1y, p0x, p0y);
    const float s3 = cross3(p0x, p0y, q1x, q1y, q0x, q0y);
    const float s4 = cross3(q1x, q1y, p1x, p1y, q0x, q0y);
    if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
    const float s5 = cross3(q1x, q1y, p1x, p1y, p0x, p0y);
    if (fabsf(s5 - s1) > kEps) {
        ax = (s5 * q0x - s1 * q1x) / (s5 - s1);
        ay = (s5 * q0y - s1 * q1y) / (s5 - s1);
    } else {
        const float a0 = p0y - p1y, b0 = p1x - p0x, c0 = p0x * p1y - p1x * p0y;
        const float a1 = q0y - q1y, b1 = q1x - q0x, c1 = q0x * q1y - q1x * q0y;
        const float D = a0 * b1 - a1 * b0;
        ax = (b0 * c1 - b1 * c0) / D;
        ay = (a1 * c0 - a0 * c1) / D;
    }
    return true;
}

// Append candidate (x, y) to cross_points[cnt] when ok: a select over the compile-time slots d <= s it can land in.
template <int s>
__device__ __forceinline__ void poly_append(bool ok, float x, float y, int& cnt, float& sx, float& sy, float (&qx)[kPoly], float (&qy)[kPoly]) {
#pragma unroll
    for (int d = 0; d <= s; ++d)
        if (ok && cnt == d) { qx[d] = x; qy[d] = y; }
    if (ok) { sx = sx + x; sy = sy + y; ++cnt; }
}

template <int i, int j>
__device__ __forceinline__ void poly_edge(const BoxG& A, const BoxG& B, int& cnt, float& sx, float& sy, float (&qx)[kPoly], float (&qy)[kPoly]) {
    constexpr int i1 = (i + 1) & 3, j1 = (j + 1) & 3;
    float x = 0.f, y = 0.f;
    const bool ok = intersection(A.px[i1], A.py[i1], A.px[i], A.py[i], B.px[j1], B.py[j1], B.px[j], B.py[j], x, y);
    poly_append<i * 4 + j>(ok, x, y, cnt, sx, sy, qx, qy);
}

// box_overlap(a, b).  Uses wave votes to cut its loops short: every lane of the wave must call it (inactive lanes are fine).
__device__ __forceinline__ float box_overlap(const BoxG& A, const BoxG& B) {
    float qx[kPoly], qy[kPoly], qk[kPoly];
#pragma unroll
    for (int d = 0; d < kPoly; ++d) { qx[d] = 0.f; qy[d] = 0.f; qk[d] = 0.f; }
    float sx = 0.f, sy = 0.f;               // poly_center: the sum in append order, then / cnt
    int cnt = 0;
    poly_edge<0, 0>(A, B, cnt, sx, sy, qx, qy); poly_edge<0, 1>(A, B, cnt, sx, sy, qx, qy);
    poly_edge<0, 2>(A, B, cnt, sx, sy, qx, qy); poly_edge<0, 3>(A, B, cnt, sx, sy, qx, qy);
    poly_edge<1, 0>(A, B, cnt, sx, sy, qx, qy); poly_edge<1, 1>(A, B, cnt, sx, sy, qx, qy);
    poly_edge<1, 2>(A, B, cnt, sx, sy, qx, qy); poly_edge<1, 3>(A, B, cnt, sx, sy, qx, qy);
    poly_edge<2, 0>(A, B, cnt, sx, sy, qx, qy); poly_edge<2, 1>(A, B, cnt, sx, sy, qx, qy);
    poly_edge<2, 2>(A, B, cnt, sx, sy, qx, qy); poly_edge<2, 3>(A, B, cnt, sx, sy, qx, qy);
    poly_edge<3, 0>(A, B, cnt, sx, sy, qx, qy); poly_edge<3, 1>(A, B, cnt, sx, sy, qx, qy);
    poly_edge<3, 2>(A, B, cnt, sx, sy, qx, qy); poly_edge<3, 3>(A, B, cnt, sx, sy, qx, qy);
    // corners: the reference appends b's corner k (if in a), then a's corner k (if in b)
    poly_append<16>(in_box2d(A, B.px[0], B.py[0]), B.px[0], B.py[0], cnt, sx, sy, qx, qy);
    poly_append<17>(in_box2d(B, A.px[0], A.py[0]), A.px[0], A.py[0], cnt, sx, sy, qx, qy);
    poly_append<18>(in_box2d(A, B.px[1], B.py[1]), B.px[1], B.py[1], cnt, sx, sy, qx, qy);
    poly_append<19>(in_box2d(B, A.px[1], A.py[1]), A.px[1], A.py[1], cnt, sx, sy, qx, qy);
    poly_append<20>(in_box2d(A, B.px[2], B.py[2]), B.px[2], B.py[2], cnt, sx, sy, qx, qy);
    poly_append<21>(in_box2d(B, A.px[2], A.py[2]), A.px[2], A.py[2], cnt, sx, sy, qx, qy);
    poly_append<22>(in_box2d(A, B.px[3], B.py[3]), B.px[3], B.py[3], cnt, sx, sy, qx, qy);
    poly_append<23>(in_box2d(B, A.px[3], A.py[3]), A.px[3], A.py[3], cnt, sx, sy, qx, qy);
    if (!__any(cnt > 0)) return 0.f;
    sx /= cnt;
    sy /= cnt;
    // point_cmp's key, computed once per point
#pragma unroll
    for (int d = 0; d < kPoly; ++d) {
        if (!__any(d < cnt)) break;
        qk[d] = atan2f(qy[d] - sy, qx[d] - sx);
    }
    // The reference bubble-sorts with point_cmp (strict >): a stable sort by key.  A stable insertion sort (shift while strictly
    // greater) yields the same permutation, so the shoelace sum below adds the same terms in the same order.
#pragma unroll
    for (int s = 1; s < kPoly; ++s) {
        if (!__any(s < cnt)) break;
        const float x = qx[s], y = qy[s], k = qk[s];
        bool moving = s < cnt;
#pragma unroll
        for (int d = s; d >= 1; --d) {
            const bool sh = moving && qk[d - 1] > k;
            if (sh) { qx[d] = qx[d - 1]; qy[d] = qy[d - 1]; qk[d] = qk[d - 1]; }
            else if (moving) { qx[d] = x; qy[d] = y; qk[d] = k; }
            moving = sh;
        }
        if (moving) { qx[0] = x; qy[0] = y; qk[0] = k; }
    }
    // shoelace about the first point
    float area = 0.f;
#pragma unroll
    for (int k = 0; k < kPoly - 1; ++k) {
        if (!__any(k < cnt - 1)) break;
        if (k < cnt - 1) {
            const float ax = qx[k] - qx[0], ay = qy[k] - qy[0];
            const float bx = qx[k + 1] - qx[0], by = qy[k + 1] - qy[0];
            area += ax * by - ay * bx;
        }
    }
    return (float)(fabsf(area) / 2.0);
}

// boxes_iou3d_gpu after the BEV overlap `ov` of boxes a and b, in its torch order: [amin, amax] = [y - h, y], avol = h * w * l
__device__ __forceinline__ float iou3d_of_overlap(float ov, float amin, float amax, float avol, float bmin, float bmax, float bvol) {
    const float max_of_min = fmaxf(amin, bmin), min_of_max = fminf(amax, bmax);
    const float oh = fmaxf(min_of_max - max_of_min, 0.f);
    const float o3 = ov * oh;
    return o3 / fmaxf(avol + bvol - o3, 1e-7f);
}

}  // namespace box3d_iou

#endif  // DISPRCNN_BOX3D_IOU_H

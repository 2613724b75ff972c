// frame_ops.hip -- the frame change between PointRCNN's two networks (gfx950): the RPN's clouds and proposals, which live in the centred,
// rotated frame InstancePointCloud made for each instance, moved back to the rectified camera frame in one launch.
//
//   reference: point_rcnn/lib/net/point_rcnn.py:296-312 (pts + mean, rotate_pc_along_y.rotate_back, the proposals through their corners),
//              structures/bounding_box_3d.py (Box3DList._split_into_corners, convert), lib/rpn's pts_depth.
//
// Every value is the fp32 expression of the torch composition (PointRCNN.proposals_to_camera_unfused) in its order; the library builds
// with -ffp-contract=off, so a * b + c * d is two products and a sum.  The rotation's cos and sin are taken in fp64 and rounded once, as
// InstancePointCloud.rotate_back does.  A workgroup works on one cloud (one workgroup per cloud up to 1024 items): each of its threads takes
// that cloud's mean and the fp64 cos and sin once, before its loop, not once per point or box -- a wave issues them once for its 64 lanes --
// and then walks the cloud's points (four at a time through 16-byte loads and stores when N is a multiple of 4) and its boxes.
// A box needs corners 0, 1, 3, 4 and 7 only: the centre is (c7 + c0) / 2, l, h, w are |c0 - c3|, |c0 - c1|, |c0 - c4|, the angle is -atan2 of the edge 0 -> 3.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_pts.h"

namespace {

constexpr int kThreads = 256;
constexpr int kItemsPerBlock = 4 * kThreads;        // 768 points (192 items of four) and 512 proposals are one workgroup

struct Frame {
    float mx, my, mz, c, s;
};

struct P3 {
    float x, y, z;
};

// (p + mean) rotated about y by -rot: x' = x * c + z * (-s), z' = x * s + z * c  (bmm with rotmat^T in rotate_back)
__device__ __forceinline__ P3 to_camera(const Frame& f, float x, float y, float z) {
    const float px = x + f.mx, py = y + f.my, pz = z + f.mz;
    return {px * f.c + pz * (-f.s), py, px * f.s + pz * f.c};
}

__device__ __forceinline__ float depth_of(const P3& p) { return sqrtf(fmaf(p.z, p.z, fmaf(p.y, p.y, p.x * p.x))); }

__device__ __forceinline__ float dist(const P3& a, const P3& b) {
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return sqrtf(dx * dx + dy * dy + dz * dz);
}

// corner of the centred box: R(ry) * (xc, yc, zc) + centre, R = [[cos, 0, sin], [0, 1, 0], [-sin, 0, cos]], then the frame change
__device__ __forceinline__ P3 corner(const Frame& f, const float* b, float cosr, float sinr, float xc, float yc, float zc) {
    const float X = (cosr * xc + sinr * zc) + b[0];
    const float Y = yc + b[1];
    const float Z = ((-sinr) * xc + cosr * zc) + b[2];
    return to_camera(f, X, Y, Z);
}

template <bool VEC4>
__global__ __launch_bounds__(kThreads) void rpn_to_camera_kernel(int N, int M, const float* __restrict__ xyz, const float* __restrict__ boxes,
                                                                 const float* __restrict__ mean, const double* __restrict__ rot,
                                                                 float* __restrict__ xyz_cam, float* __restrict__ depth,
                                                                 float* __restrict__ boxes_cam) {
    const int b = blockIdx.x;
    const double a = -rot[b];
    const Frame f = {mean[b * 3 + 0], mean[b * 3 + 1], mean[b * 3 + 2], (float)cos(a), (float)sin(a)};
    const int P = VEC4 ? N / 4 : N;                                  // point items of this cloud
    const float* src = xyz + (int64_t)b * N * 3;
    float* dst = xyz_cam + (int64_t)b * N * 3;
    float* dd = depth + (int64_t)b * N;
    for (int i = blockIdx.y * kThreads + threadIdx.x; i < P + M; i += gridDim.y * kThreads) {
        if (i < P) {
            if (VEC4) {
                const float4* s4 = reinterpret_cast<const float4*>(src) + (int64_t)i * 3;
                const float4 v0 = s4[0], v1 = s4[1], v2 = s4[2];
                const P3 p0 = to_camera(f, v0.x, v0.y, v0.z), p1 = to_camera(f, v0.w, v1.x, v1.y);
                const P3 p2 = to_camera(f, v1.z, v1.w, v2.x), p3 = to_camera(f, v2.y, v2.z, v2.w);
                float4* d4 = reinterpret_cast<float4*>(dst) + (int64_t)i * 3;
                d4[0] = make_float4(p0.x, p0.y, p0.z, p1.x);
                d4[1] = make_float4(p1.y, p1.z, p2.x, p2.y);
                d4[2] = make_float4(p2.z, p3.x, p3.y, p3.z);
                reinterpret_cast<float4*>(dd)[i] = make_float4(depth_of(p0), depth_of(p1), depth_of(p2), depth_of(p3));
            } else {
                const P3 p = to_camera(f, src[i * 3 + 0], src[i * 3 + 1], src[i * 3 + 2]);
                dst[i * 3 + 0] = p.x; dst[i * 3 + 1] = p.y; dst[i * 3 + 2] = p.z;
                dd[i] = depth_of(p);
            }
        } else {
            const int64_t m = (int64_t)b * M + (i - P);
            const float* bx = boxes + m * 7;
            const float h = bx[3], w = bx[4], l = bx[5];
            const float cosr = cosf(bx[6]), sinr = sinf(bx[6]);
            const float xl = -l / 2, xh = l / 2, zl = -w / 2, zh = w / 2;
            const P3 c0 = corner(f, bx, cosr, sinr, xl, 0.f, zh);
            const P3 c1 = corner(f, bx, cosr, sinr, xl, -h, zh);
            const P3 c3 = corner(f, bx, cosr, sinr, xh, 0.f, zh);
            const P3 c4 = corner(f, bx, cosr, sinr, xl, 0.f, zl);
            const P3 c7 = corner(f, bx, cosr, sinr, xh, 0.f, zl);
            float* o = boxes_cam + m * 7;
            o[0] = (c7.x + c0.x) / 2; o[1] = (c7.y + c0.y) / 2; o[2] = (c7.z + c0.z) / 2;
            o[3] = dist(c0, c1); o[4] = dist(c0, c4); o[5] = dist(c0, c3);
            o[6] = -atan2f(c3.z - c0.z, c3.x - c0.x);
        }
    }
}

}  // namespace

extern "C" int drc_rpn_to_camera_fwd(int B, int N, int M, const float* xyz, const float* boxes, const float* mean, const double* rot,
                                     float* xyz_cam, float* depth, float* boxes_cam, void* stream) {
    if (B < 0 || N < 0 || M < 0) return -2;
    if (B == 0 || (N == 0 && M == 0)) return 0;
    if (!mean || !rot || (N > 0 && (!xyz || !xyz_cam || !depth)) || (M > 0 && (!boxes || !boxes_cam))) return -1;
    if ((int64_t)B * N * 3 > INT32_MAX || (int64_t)B * M * 7 > INT32_MAX || (int64_t)N + M > 65535LL * kItemsPerBlock) return -2;
    const bool vec4 = (N & 3) == 0 && (((uintptr_t)xyz | (uintptr_t)xyz_cam | (uintptr_t)depth) & 15) == 0;
    const int items = (vec4 ? N / 4 : N) + M;
    const dim3 grid((unsigned)B, (unsigned)((items + kItemsPerBlock - 1) / kItemsPerBlock));
    if (vec4)
        hipLaunchKernelGGL(rpn_to_camera_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, N, M, xyz, boxes, mean, rot, xyz_cam, depth,
                           boxes_cam);
    else
        hipLaunchKernelGGL(rpn_to_camera_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, N, M, xyz, boxes, mean, rot, xyz_cam, depth,
                           boxes_cam);
    return (int)hipGetLastError();
}

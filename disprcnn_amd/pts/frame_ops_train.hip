// frame_ops_train.hip -- the way into the cloud frame (gfx950): the twin of frame_ops.hip's drc_rpn_to_camera_fwd, used by PointRCNN's
// training input for the eight corners of each matched ground-truth box.
//
//   reference: point_rcnn/lib/net/point_rcnn.py:145-180 (pts * scale, the flip of x, rotate_pc_along_y, the mean subtracted).
//
// A camera-frame point times `scale`, x negated when flipped, rotated about y by rot (the signed angle InstancePointCloud used), minus the
// cloud's mean: x' = x * c + z * (-s), z' = x * s + z * c as rotate_pc_along_y, in fp32 in that order (the library builds with
// -ffp-contract=off); cos and sin are taken in fp64 and rounded once.  One workgroup row per cloud, plain C++, no LDS.  It lives in a file
// of its own so that frame_ops.hip stays the two instances of one kernel its resource-usage test counts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_pts.h"

namespace {

constexpr int kThreads = 256;
constexpr int kItemsPerBlock = 4 * kThreads;

__global__ __launch_bounds__(kThreads) void camera_to_rpn_kernel(int K, const float* __restrict__ xyz, float scale, int flip,
                                                                 const float* __restrict__ mean, const double* __restrict__ rot,
                                                                 float* __restrict__ out) {
    const int b = blockIdx.x;
    const double a = rot[b];
    const float mx = mean[b * 3 + 0], my = mean[b * 3 + 1], mz = mean[b * 3 + 2];
    const float c = (float)cos(a), s = (float)sin(a), ns = (float)(-sin(a));
    const float* src = xyz + (int64_t)b * K * 3;
    float* dst = out + (int64_t)b * K * 3;
    for (int i = blockIdx.y * kThreads + threadIdx.x; i < K; i += gridDim.y * kThreads) {
        float x = src[i * 3 + 0] * scale;
        const float y = src[i * 3 + 1] * scale, z = src[i * 3 + 2] * scale;
        if (flip) x = -x;
        dst[i * 3 + 0] = (x * c + z * ns) - mx;
        dst[i * 3 + 1] = y - my;
        dst[i * 3 + 2] = (x * s + z * c) - mz;
    }
}

}  // namespace

extern "C" int drc_camera_to_rpn_fwd(int B, int K, const float* xyz, float scale, int flip, const float* mean, const double* rot, float* out,
                                     void* stream) {
    if (B < 0 || K < 0) return -2;
    if (B == 0 || K == 0) return 0;
    if (!xyz || !mean || !rot || !out) return -1;
    if ((int64_t)B * K * 3 > INT32_MAX || (int64_t)K > 65535LL * kItemsPerBlock) return -2;
    const dim3 grid((unsigned)B, (unsigned)((K + kItemsPerBlock - 1) / kItemsPerBlock));
    hipLaunchKernelGGL(camera_to_rpn_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, K, xyz, scale, flip ? 1 : 0, mean, rot, out);
    return (int)hipGetLastError();
}

// match2d.hip -- PointRCNN.match_targets_to_proposals for every image of the batch in one launch (gfx950).
//
//   reference: point_rcnn/lib/net/point_rcnn.py:87-95 (match_targets_to_proposals), structures/boxlist_ops.py:101-136 (boxlist_iou),
//              modeling/matcher.py (Matcher without low-quality matches).
//
// One thread per left proposal walks the ground-truth 2D boxes of its own image: the IoU in fp32 in the reference's expression order
// (TO_REMOVE = 1, inter / (area1 + area2 - inter); the library builds with -ffp-contract=off), the maximum with ties to the lowest index
// (torch's max over dim 0), then the Matcher's thresholds.  It writes the matched index (int64: -1 below the low threshold, -2 between
// the two) and the matched target's `row` numbers (its 3D box), taken at the index clamped at zero as the reference's
// target[matched_idxs.clamp(min=0)].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_pts.h"

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void match_targets_kernel(int R, int G, const float* __restrict__ boxes, const int32_t* __restrict__ span,
                                                                 const float* __restrict__ gt, const float* __restrict__ gt_rows, int row,
                                                                 float high, float low, int64_t* __restrict__ matched,
                                                                 float* __restrict__ out_rows) {
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= R) return;
    int first = span[r * 2 + 0], n = span[r * 2 + 1];
    if (first < 0 || n <= 0 || first >= G) { first = 0; n = 0; }
    if (n > G - first) n = G - first;
    const float x1 = boxes[r * 4 + 0], y1 = boxes[r * 4 + 1], x2 = boxes[r * 4 + 2], y2 = boxes[r * 4 + 3];
    const float area2 = (x2 - x1 + 1.f) * (y2 - y1 + 1.f);
    float best = -1.f;
    int arg = 0;
    for (int g = 0; g < n; ++g) {
        const float* t = gt + (int64_t)(first + g) * 4;
        const float area1 = (t[2] - t[0] + 1.f) * (t[3] - t[1] + 1.f);
        float w = (fminf(t[2], x2) - fmaxf(t[0], x1)) + 1.f;
        float h = (fminf(t[3], y2) - fmaxf(t[1], y1)) + 1.f;
        w = w < 0.f ? 0.f : w;
        h = h < 0.f ? 0.f : h;
        const float inter = w * h;
        const float iou = inter / ((area1 + area2) - inter);
        if (iou > best || (g == 0)) { best = iou; arg = g; }
    }
    int64_t m = arg;
    if (n == 0 || best < low) m = -1;
    else if (best < high) m = -2;
    matched[r] = m;
    if (n > 0) {
        const int64_t src = (int64_t)(first + (m < 0 ? 0 : m)) * row;
        for (int k = 0; k < row; ++k) out_rows[(int64_t)r * row + k] = gt_rows[src + k];
    } else {
        for (int k = 0; k < row; ++k) out_rows[(int64_t)r * row + k] = 0.f;
    }
}

}  // namespace

extern "C" int drc_match_targets_fwd(int R, int G, const float* boxes, const int32_t* span, const float* gt, const float* gt_rows, int row,
                                     float high, float low, int64_t* matched, float* out_rows, void* stream) {
    if (R < 0 || G < 0 || row < 0) return -2;
    if (R == 0) return 0;
    if (!boxes || !span || !matched || (row > 0 && !out_rows) || (G > 0 && (!gt || (row > 0 && !gt_rows)))) return -1;
    if ((int64_t)R * (row > 4 ? row : 4) > INT32_MAX) return -2;
    hipLaunchKernelGGL(match_targets_kernel, dim3((unsigned)((R + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, R, G, boxes,
                       span, gt, gt_rows, row, high, low, matched, out_rows);
    return (int)hipGetLastError();
}

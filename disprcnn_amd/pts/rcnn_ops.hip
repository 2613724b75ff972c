// rcnn_ops.hip -- PointRCNN's second network (gfx950): ROI pooling fused with the canonical transform, and the RCNN box decode.
//
//   reference: point_rcnn/lib/net/rcnn_net.py (forward, ROI_SAMPLE_JIT eval branch), utils/roipool3d (roipool3d_gpu, enlarge_box3d),
//              utils/kitti_utils.py (rotate_pc_along_y_torch, boxes3d_to_bev_torch), net/rcnn_inference.py,
//              utils/bbox_transform.py (decode_bbox_target with get_xz_fine and get_ry_fine).
//
// Every value is the reference's fp32 expression in its order (the library builds with -ffp-contract=off).  The schedules are ours:
//   - pooling: one workgroup per (cloud, ROI).  The box is enlarged in registers, the first S in-box points are selected as roipool3d
//     does (box3d_pt.h) and the list is filled cyclically in LDS (S indices, sized by the launch).  The outputs are then written in the layouts the shared MLPs read:
//     canonical xyz point-major [R,S,3], and the channel-major rows [R,3+E,S] and [R,C,S] straight from the RPN's channel-major
//     features [B,C,N] -- a wave writes one channel row along S with 16-byte stores, its gathers hit one 4 N-byte row that stays in
//     cache.  The [B,N,E+C] concat, the [B,M,S,3+E+C] point-major tensor and its transposes never exist;
//   - decode: one thread per ROI; bins by first-maximum argmax, the rotation back by the ROI's angle, BEV form and sigmoid together.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_pts.h"
#include "box3d_pt.h"

namespace {

using box3d_pt::kMaxPoolSamples;
using box3d_pt::kPoolThreads;
using box3d_pt::gather_rows;             // shared with proposal_target.hip

__global__ __launch_bounds__(kPoolThreads) void pool_canonical_kernel(int N, int M, int C, int S, int E, const float* __restrict__ xyz,
                                                                      const float* __restrict__ feat, const float* __restrict__ mask,
                                                                      const float* __restrict__ depth, const float* __restrict__ rois,
                                                                      float extra, float extra2, float* __restrict__ oxyz,
                                                                      float* __restrict__ opts, float* __restrict__ ofeat,
                                                                      int32_t* __restrict__ empty_flag) {
    extern __shared__ __attribute__((aligned(16))) int32_t sidx[];          // S indices (the launch sizes it): 2 KB at S = 512
    __shared__ int wcnt[kPoolThreads / 64];
    const int bm = blockIdx.x, b = bm / M;
    const int tid = threadIdx.x;
    const float* roi = rois + (int64_t)bm * 7;
    // enlarge_box3d: h, w, l + 2 * extra_width, bottom y + extra_width; the centre and the angle are the ROI's own
    const float bx[7] = {roi[0], roi[1] + extra, roi[2], roi[3] + extra2, roi[4] + extra2, roi[5] + extra2, roi[6]};
    const float cosa = cosf(bx[6]), sina = sinf(bx[6]);
    const float* p = xyz + (int64_t)b * N * 3;
    const int cnt = box3d_pt::select_in_box(N, S, p, bx, cosa, sina, sidx, wcnt);      // block-uniform
    const bool empty = cnt == 0;
    if (tid == 0) empty_flag[bm] = empty ? 1 : 0;
    const int have = min(cnt, S);
    if (!empty) {
        for (int s = have + tid; s < S; s += kPoolThreads) sidx[s] = sidx[s % have];       // reads < have, writes >= have
        __syncthreads();
    }
    // canonical coordinates: (p - centre) rotated about y by the ROI's angle (rotate_pc_along_y_torch); an empty ROI pools zeros
    float* ox = oxyz + (int64_t)bm * S * 3;
    float* op = opts + (int64_t)bm * (3 + E) * S;
    const float* mb = mask + (int64_t)b * N;
    const float* db = depth + (int64_t)b * N;              // read only when E == 2
    for (int s = tid; s < S; s += kPoolThreads) {
        float px = 0.f, py = 0.f, pz = 0.f, mv = 0.f, dv = 0.f;
        if (!empty) {
            const int src = sidx[s];
            px = p[(int64_t)src * 3 + 0]; py = p[(int64_t)src * 3 + 1]; pz = p[(int64_t)src * 3 + 2];
            mv = mb[src];
            if (E > 1) dv = db[src] / 70.0f - 0.5f;
        }
        const float dx = px - roi[0], dy = py - roi[1], dz = pz - roi[2];
        const float cx = dx * cosa + dz * (-sina);
        const float cz = dx * sina + dz * cosa;
        ox[s * 3 + 0] = cx; ox[s * 3 + 1] = dy; ox[s * 3 + 2] = cz;
        op[s] = cx; op[S + s] = dy; op[2 * S + s] = cz;
        op[3 * S + s] = mv;
        if (E > 1) op[4 * S + s] = dv;
    }
    if (C > 0) gather_rows(C, N, S, empty ? nullptr : feat + (int64_t)b * C * N, sidx, ofeat + (int64_t)bm * C * S);
}

// ---- RCNN decode
struct RcnnDecodeArgs {
    int per_loc_bin_num, loc_y_bin_num, num_head_bin, y_by_bin, R;
    float loc_bin_size, half_bin, loc_scope, loc_y_bin_size, half_y_bin, loc_y_scope, angle_per_class, half_angle, quarter_pi, ah, aw, al;
};

__device__ __forceinline__ int first_argmax(const float* p, int n) {
    int best = 0;
    float bv = p[0];
    for (int i = 1; i < n; ++i)
        if (p[i] > bv) { bv = p[i]; best = i; }
    return best;
}

__global__ __launch_bounds__(256) void rcnn_decode_kernel(int64_t total, const float* __restrict__ rois, const float* __restrict__ reg,
                                                          const float* __restrict__ cls, float* __restrict__ boxes, float* __restrict__ bev,
                                                          float* __restrict__ score, const RcnnDecodeArgs d) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const float* r = reg + t * d.R;
    const float* roi = rois + t * 7;
    const int nb = d.per_loc_bin_num;
    const int xb = first_argmax(r, nb), zb = first_argmax(r + nb, nb);
    float pos_x = (float)xb * d.loc_bin_size + d.half_bin - d.loc_scope;
    float pos_z = (float)zb * d.loc_bin_size + d.half_bin - d.loc_scope;
    const float x_res = r[2 * nb + xb] * d.loc_bin_size, z_res = r[3 * nb + zb] * d.loc_bin_size;
    pos_x = pos_x + x_res;
    pos_z = pos_z + z_res;
    int off = 4 * nb;
    float pos_y;
    if (d.y_by_bin) {
        const int yn = d.loc_y_bin_num;
        const int yb = first_argmax(r + off, yn);
        const float y_res = r[off + yn + yb] * d.loc_y_bin_size;
        pos_y = (float)yb * d.loc_y_bin_size + d.half_y_bin - d.loc_y_scope + y_res;
        pos_y = pos_y + roi[1];
        off += 2 * yn;
    } else {
        pos_y = roi[1] + r[off];
        off += 1;
    }
    const int rbin = first_argmax(r + off, d.num_head_bin);
    const float ry_res = r[off + d.num_head_bin + rbin] * d.half_angle;
    float ry = ((float)rbin * d.angle_per_class + d.half_angle) + ry_res - d.quarter_pi;
    off += 2 * d.num_head_bin;
    const float hh = r[off] * d.ah + d.ah, ww = r[off + 1] * d.aw + d.aw, ll = r[off + 2] * d.al + d.al;
    // rotate_pc_along_y_torch(box, -roi_ry), ry + roi_ry, then the ROI's centre on x and z
    const float roi_ry = roi[6], na = -roi_ry;
    const float cosa = cosf(na), sina = sinf(na);
    const float rx = pos_x * cosa + pos_z * (-sina);
    const float rz = pos_x * sina + pos_z * cosa;
    ry = ry + roi_ry;
    const float x = rx + roi[0], z = rz + roi[2];
    float* o = boxes + t * 7;
    o[0] = x; o[1] = pos_y; o[2] = z; o[3] = hh; o[4] = ww; o[5] = ll; o[6] = ry;
    const float half_l = ll / 2.f, half_w = ww / 2.f;
    float* e = bev + t * 5;
    e[0] = x - half_l; e[1] = z - half_w; e[2] = x + half_l; e[3] = z + half_w; e[4] = ry;
    score[t] = 1.f / (1.f + expf(-cls[t]));
}

}  // namespace

extern "C" int drc_rcnn_pool_canonical_fwd(int B, int N, int M, int C, int S, const float* rpn_xyz, const float* feat, const float* seg_mask,
                                           const float* pts_depth, int use_depth, const float* rois, float extra_width, float extra_width2, float* xyz,
                                           float* pts, float* ofeat, int32_t* empty_flag, void* stream) {
    if (B < 0 || N < 0 || M < 0 || C < 0 || S < 1 || S > kMaxPoolSamples) return -2;
    const int64_t blocks = (int64_t)B * M;
    if (blocks == 0) return 0;
    if (blocks > INT32_MAX) return -2;
    if (!rois || !empty_flag || (N > 0 && (!rpn_xyz || !seg_mask || (use_depth && !pts_depth))) || (N > 0 && C > 0 && !feat)) return -1;
    if (S > 0 && (!xyz || !pts || (C > 0 && !ofeat))) return -1;
    hipLaunchKernelGGL(pool_canonical_kernel, dim3((unsigned)blocks), dim3(kPoolThreads), (size_t)((S + 3) & ~3) * sizeof(int32_t), (hipStream_t)stream, N, M, C, S,
                       use_depth ? 2 : 1, rpn_xyz, feat, seg_mask, pts_depth, rois, extra_width, extra_width2, xyz, pts, ofeat, empty_flag);
    return (int)hipGetLastError();
}

extern "C" int drc_rcnn_decode_boxes(int64_t n, int R, const float* rois, const float* reg, const float* cls, int per_loc_bin_num,
                                     int loc_y_bin_num, int num_head_bin, int y_by_bin, float loc_bin_size, float half_bin, float loc_scope,
                                     float loc_y_bin_size, float half_y_bin, float loc_y_scope, float angle_per_class, float half_angle,
                                     float quarter_pi, float anchor_h, float anchor_w, float anchor_l, float* boxes, float* bev,
                                     float* norm_score, void* stream) {
    if (n < 0 || per_loc_bin_num < 1 || num_head_bin < 1 || (y_by_bin && loc_y_bin_num < 1)) return -1;
    if (R != per_loc_bin_num * 4 + (y_by_bin ? 2 * loc_y_bin_num : 1) + 2 * num_head_bin + 3) return -2;
    if (n == 0) return 0;
    if (!rois || !reg || !cls || !boxes || !bev || !norm_score) return -1;
    const RcnnDecodeArgs d = {per_loc_bin_num, loc_y_bin_num, num_head_bin, y_by_bin ? 1 : 0, R, loc_bin_size, half_bin, loc_scope,
                              loc_y_bin_size, half_y_bin, loc_y_scope, angle_per_class, half_angle, quarter_pi, anchor_h, anchor_w, anchor_l};
    const int64_t blocks = (n + 255) / 256;
    if (blocks > INT32_MAX) return -2;
    hipLaunchKernelGGL(rcnn_decode_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n, rois, reg, cls, boxes, bev,
                       norm_score, d);
    return (int)hipGetLastError();
}

// proposal_target.hip -- PointRCNN's ProposalTargetLayer (gfx950): the sampling of the RCNN stage's training ROIs and their pooling,
// augmentation, canonical transform and labels, in two kernels without a host read.
//
//   reference: point_rcnn/lib/rpn/proposal_target_layer.py (sample_rois_for_rcnn, sample_bg_inds, aug_roi_by_noise_torch,
//              random_aug_box3d, data_augmentation, forward), utils/iou3d (boxes_iou3d_gpu), utils/roipool3d (roipool3d_gpu),
//              utils/kitti_utils.py (rotate_pc_along_y_torch, enlarge_box3d).
//
// Every value is the reference's fp32 expression in its order (the library builds with -ffp-contract=off).  Every random decision reads
// one fp32 uniform of `draws` (layout: include/disprcnn_pts.h); the schedules are ours:
//   - sampling: one workgroup per cloud.  IoU3D of the M candidates against the cloud's N boxes, a candidate per lane (row maximum and
//     first arg-max in LDS); wave 0 builds the three class lists in index order by ballot + popcount prefix; the foreground choice is
//     a rank by key (ties to the lower index); then one lane per slot runs the noise loop.  box_overlap votes across the wave, so every
//     lane of a wave that holds a slot makes each call, and lanes that are done ignore the result;
//   - pooling: one workgroup per (cloud, slot), the training form of rcnn_ops.hip's pool_canonical_kernel: the same selection
//     (box3d_pt.h) and row writers, with the slot's rotation, scale and flip applied to the pooled coordinates, the ROI and its ground
//     truth before the canonical transform, and the labels written by the same workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_pts.h"
#include "box3d_iou.h"
#include "box3d_pt.h"

namespace {

using namespace box3d_iou;
using box3d_pt::gather_rows;
using box3d_pt::kMaxPoolSamples;
using box3d_pt::kPoolThreads;

constexpr int kSampleThreads = 256;
constexpr int kMaxCand = 1024;              // candidates per cloud: 5 LDS words each (row maximum, arg-max, three class lists): 20 KB
constexpr int kMaxSlots = kSampleThreads;   // one lane per slot
constexpr int kCounts = 5;                  // per cloud: fg, hard bg, easy bg candidates, fg slots taken, the no-candidate flag
constexpr float kPi = 3.14159265358979323846f;         // np.pi as the fp32 scalar torch makes of it
constexpr float kTwoPi = 6.28318530717958647692f;

// random_aug_box3d's range_config [pos, hwl, angle] ('multiple'), the Python doubles rounded to fp32 as torch's scalar operands are
__constant__ float kRange[5][3] = {{0.2f, 0.1f, (float)(3.14159265358979323846 / 12)},
                                   {0.3f, 0.15f, (float)(3.14159265358979323846 / 12)},
                                   {0.5f, 0.15f, (float)(3.14159265358979323846 / 9)},
                                   {0.8f, 0.15f, (float)(3.14159265358979323846 / 6)},
                                   {1.0f, 0.15f, (float)(3.14159265358979323846 / 3)}};
constexpr float kSingleHwlDiv = (float)(0.5 / 0.15);
constexpr float kSingleAngDiv = (float)(0.5 / (3.14159265358979323846 / 12));

struct Box3 {                               // what boxes_iou3d_gpu derives from one [x, y, z, h, w, l, ry]
    BoxG g;
    float ymin, ymax, vol;
};

__device__ __forceinline__ Box3 box3_of(const float* b) {
    Box3 r;
    r.g = box_geom7(b);
    r.ymin = b[1] - b[3];
    r.ymax = b[1];
    r.vol = b[3] * b[4] * b[5];
    return r;
}

// every lane of the wave must call it (box_overlap)
__device__ __forceinline__ float iou3d(const Box3& a, const Box3& b) {
    return iou3d_of_overlap(box_overlap(a.g, b.g), a.ymin, a.ymax, a.vol, b.ymin, b.ymax, b.vol);
}

// min(floor(u * n), n - 1), held inside [0, n) whatever the draw holds
__device__ __forceinline__ int pick_index(float u, int n) { return (int)fminf(fmaxf(floorf(u * (float)n), 0.f), (float)(n - 1)); }

__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }        // torch.sign

struct SampleArgs {
    int M, N, P, T, fg_per_image, method;   // method 0: 'multiple', 1: 'single'
    float fg_thresh, bg_thresh, bg_thresh_lo;
    double hard_bg_ratio;
    int64_t draw_stride;
};

__global__ __launch_bounds__(kSampleThreads) void sample_rois_kernel(const SampleArgs a, const float* __restrict__ cand,
                                                                     const float* __restrict__ gt, const float* __restrict__ draws,
                                                                     float* __restrict__ orois, float* __restrict__ ogt,
                                                                     float* __restrict__ oiou, int32_t* __restrict__ osrc,
                                                                     int32_t* __restrict__ oiter, int32_t* __restrict__ counts) {
    __shared__ float s_max[kMaxCand];
    __shared__ int s_asg[kMaxCand];
    __shared__ int s_list[3][kMaxCand];     // fg, hard bg, easy bg candidates in index order
    __shared__ int s_cnt[3];
    __shared__ int s_sel[kMaxSlots];        // the fg candidates taken, in key order
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = a.M, N = a.N, P = a.P, T = a.T;
    const float* cr = cand + (int64_t)b * M * 7;
    const float* cg = gt + (int64_t)b * N * 7;
    const float* dr = draws + (int64_t)b * a.draw_stride;

    // 1. IoU3D against the cloud's boxes: torch.max(iou3d, dim=1), the first maximum
    for (int base = 0; base < M; base += kSampleThreads) {          // block-uniform: every lane makes every call
        const int i = base + tid;
        const Box3 A = box3_of(cr + (int64_t)min(i, M - 1) * 7);
        float best = 0.f;
        int arg = 0;
        for (int n = 0; n < N; ++n) {
            const Box3 G = box3_of(cg + (int64_t)n * 7);
            const float v = iou3d(A, G);
            if (n == 0 || v > best) { best = v; arg = n; }
        }
        if (i < M) { s_max[i] = best; s_asg[i] = arg; }
    }
    __syncthreads();

    // 2. the three classes, in index order
    if (wave == 0) {
        int c0 = 0, c1 = 0, c2 = 0;
        const uint64_t below = (1ull << lane) - 1ull;
        for (int base = 0; base < M; base += 64) {
            const int i = base + lane;
            const bool ok = i < M;
            const float v = ok ? s_max[i] : 0.f;
            const bool fg = ok && v >= a.fg_thresh;
            const bool hard = ok && v < a.bg_thresh && v >= a.bg_thresh_lo;
            const bool easy = ok && v < a.bg_thresh_lo;
            const uint64_t bf = __ballot(fg), bh = __ballot(hard), be = __ballot(easy);
            if (fg) s_list[0][c0 + __popcll(bf & below)] = i;
            if (hard) s_list[1][c1 + __popcll(bh & below)] = i;
            if (easy) s_list[2][c2 + __popcll(be & below)] = i;
            c0 += __popcll(bf); c1 += __popcll(bh); c2 += __popcll(be);
        }
        if (lane == 0) { s_cnt[0] = c0; s_cnt[1] = c1; s_cnt[2] = c2; }
    }
    __syncthreads();
    const int n_fg = s_cnt[0], n_hard = s_cnt[1], n_easy = s_cnt[2], n_bg = n_hard + n_easy;
    const bool none = n_fg == 0 && n_bg == 0;
    const int fg_taken = n_fg > 0 ? (n_bg > 0 ? min(a.fg_per_image, n_fg) : P) : 0;
    const int bg_slots = P - fg_taken;
    const int hard_slots = (n_hard > 0 && n_easy > 0) ? (int)((double)bg_slots * a.hard_bg_ratio) : (n_hard > 0 ? bg_slots : 0);

    // 3. randperm(fg)[:k]: the k smallest keys in key order, ties to the lower index
    if (n_fg > 0 && n_bg > 0) {
        for (int e = tid; e < n_fg; e += kSampleThreads) {
            const int c = s_list[0][e];
            const float kc = dr[c];
            int rank = 0;
            for (int e2 = 0; e2 < n_fg; ++e2) {
                const float k2 = dr[s_list[0][e2]];
                rank += (k2 < kc || (k2 == kc && e2 < e)) ? 1 : 0;
            }
            if (rank < fg_taken) s_sel[rank] = c;
        }
    }
    __syncthreads();
    if (wave * 64 >= P) return;             // a wave without a slot; no barrier follows

    // 4. slots: foreground, hard background, easy background
    const bool active = tid < P;
    const int j = min(tid, P - 1);
    const float pick = dr[M + j];
    int src;
    if (none) src = j % M;
    else if (j < fg_taken) src = n_bg > 0 ? s_sel[j] : s_list[0][pick_index(pick, n_fg)];
    else if (j < fg_taken + hard_slots) src = s_list[1][pick_index(pick, n_hard)];
    else src = s_list[2][pick_index(pick, n_easy)];
    const int times = (!active || none) ? 0 : (j < fg_taken ? T : min(T, 1));

    // 5. aug_roi_by_noise_torch
    float roi[7], g[7], aug[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        roi[k] = cr[(int64_t)src * 7 + k];
        g[k] = cg[(int64_t)s_asg[src] * 7 + k];
        aug[k] = roi[k];
    }
    const Box3 G = box3_of(g);
    const float* nz = dr + M + P + (int64_t)j * T * 9;
    float temp_iou = 0.f;
    int cnt = 0;
    bool keep = true;
    while (__any(temp_iou < a.fg_thresh && cnt < times)) {
        const bool run = temp_iou < a.fg_thresh && cnt < times;
        float c7[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) c7[k] = roi[k];
        bool kp = true;
        if (run) {
            const float* u = nz + cnt * 9;
            kp = (double)u[0] < 0.2;        // np.random.rand() < 0.2: a double compare
            if (!kp) {
                if (a.method == 0) {
                    const int idx = pick_index(u[1], 5);
                    const float r0 = kRange[idx][0], r1 = kRange[idx][1], r2 = kRange[idx][2];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        c7[k] = roi[k] + ((u[2 + k] - 0.5f) / 0.5f) * r0;
                        c7[3 + k] = roi[3 + k] * (((u[5 + k] - 0.5f) / 0.5f) * r1 + 1.0f);
                    }
                    c7[6] = roi[6] + ((u[8] - 0.5f) / 0.5f) * r2;
                } else {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        c7[k] = roi[k] + (u[2 + k] - 0.5f);
                        c7[3 + k] = roi[3 + k] * ((u[5 + k] - 0.5f) / kSingleHwlDiv + 1.0f);
                    }
                    c7[6] = roi[6] + (u[8] - 0.5f) / kSingleAngDiv;
                }
            }
        }
        const Box3 A = box3_of(c7);
        const float v = iou3d(A, G);
        if (run) {
#pragma unroll
            for (int k = 0; k < 7; ++k) aug[k] = c7[k];
            keep = kp;
            temp_iou = v;
            ++cnt;
        }
    }
    if (active) {
        const int64_t o = (int64_t)b * P + tid;
#pragma unroll
        for (int k = 0; k < 7; ++k) { orois[o * 7 + k] = aug[k]; ogt[o * 7 + k] = g[k]; }
        oiou[o] = (cnt == 0 || keep) ? s_max[src] : temp_iou;
        osrc[o] = src;
        oiter[o] = cnt;
    }
    if (tid == 0) {
        int32_t* c = counts + (int64_t)b * kCounts;
        c[0] = n_fg; c[1] = n_hard; c[2] = n_easy; c[3] = fg_taken; c[4] = none ? 1 : 0;
    }
}

struct PoolTargetArgs {
    int N, P, C, S, E, aug;
    float extra, extra2, rot_range, reg_fg, cls_fg, cls_bg;        // rot_range: np.pi / AUG_ROT_RANGE rounded to fp32
    int64_t draw_stride;
};

// rotate_pc_along_y_torch of one (x, z)
__device__ __forceinline__ void rot_y(float& x, float& z, float cosa, float sina) {
    const float nx = x * cosa + z * (-sina);
    const float nz = x * sina + z * cosa;
    x = nx;
    z = nz;
}

// torch's `%` (remainder with the divisor's sign) of fp32 operands
__device__ __forceinline__ float py_mod(float v, float d) {
    float m = fmodf(v, d);
    if (m != 0.f && ((d < 0.f) != (m < 0.f))) m += d;
    return m;
}

__global__ __launch_bounds__(kPoolThreads) void pool_target_kernel(const PoolTargetArgs a, const float* __restrict__ xyz,
                                                                   const float* __restrict__ feat, const float* __restrict__ mask,
                                                                   const float* __restrict__ depth, const float* __restrict__ rois,
                                                                   const float* __restrict__ gts, const float* __restrict__ ious,
                                                                   const int32_t* __restrict__ counts, const float* __restrict__ aug_draws,
                                                                   float* __restrict__ oxyz, float* __restrict__ opts,
                                                                   float* __restrict__ ofeat, int32_t* __restrict__ empty_flag,
                                                                   float* __restrict__ oroi, float* __restrict__ ogt,
                                                                   int64_t* __restrict__ cls_label, int64_t* __restrict__ reg_valid) {
    extern __shared__ __attribute__((aligned(16))) int32_t sidx[];          // S indices (the launch sizes it)
    __shared__ int wcnt[kPoolThreads / 64];
    const int bm = blockIdx.x, b = bm / a.P, slot = bm - b * a.P;
    const int tid = threadIdx.x, N = a.N, S = a.S, E = a.E;
    float r[7], g[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        r[k] = rois[(int64_t)bm * 7 + k];
        g[k] = gts[(int64_t)bm * 7 + k];
    }
    // the pooling box: the noise-augmented ROI enlarged (enlarge_box3d), before the data augmentation
    const float bx[7] = {r[0], r[1] + a.extra, r[2], r[3] + a.extra2, r[4] + a.extra2, r[5] + a.extra2, r[6]};
    const float* p = xyz + (int64_t)b * N * 3;
    const int cnt = box3d_pt::select_in_box(N, S, p, bx, cosf(bx[6]), sinf(bx[6]), sidx, wcnt);       // block-uniform
    const bool empty = cnt == 0;
    const int have = min(cnt, S);
    if (!empty) {
        for (int s = have + tid; s < S; s += kPoolThreads) sidx[s] = sidx[s % have];       // reads < have, writes >= have
        __syncthreads();
    }
    // data_augmentation of the ROI and its ground truth: rotation about y, scale, flip
    float ca = 1.f, sa = 0.f, sc = 1.f, fx = 1.f;
    if (a.aug) {
        const float* u = aug_draws + (int64_t)b * a.draw_stride + slot * 3;
        const float angle = (u[0] - 1.0f) * a.rot_range;               // (rand - 0.5 / 0.5) * (pi / AUG_ROT_RANGE), as the reference evaluates it
        float beta = atan2f(g[2], g[0]);
        const float gt_alpha = -sgn(beta) * kPi / 2.f + beta + g[6];
        beta = atan2f(r[2], r[0]);
        const float roi_alpha = -sgn(beta) * kPi / 2.f + beta + r[6];
        ca = cosf(angle);
        sa = sinf(angle);
        rot_y(g[0], g[2], ca, sa);
        rot_y(r[0], r[2], ca, sa);
        beta = atan2f(g[2], g[0]);
        g[6] = sgn(beta) * kPi / 2.f + gt_alpha - beta;
        beta = atan2f(r[2], r[0]);
        r[6] = sgn(beta) * kPi / 2.f + roi_alpha - beta;
        sc = ((u[1] - 0.5f) / 0.5f) * 0.05f + 1.0f;
#pragma unroll
        for (int k = 0; k < 6; ++k) { g[k] = g[k] * sc; r[k] = r[k] * sc; }
        const float flip = sgn(u[2] - 0.5f);                           // 0 (u == 0.5 exactly) counts as no flip
        fx = flip == -1.f ? -1.f : 1.f;
        const float keep_w = flip == -1.f ? 0.f : 1.f, flip_w = flip == -1.f ? 1.f : 0.f;
        g[0] = g[0] * fx;
        g[6] = keep_w * g[6] + flip_w * (sgn(g[6]) * kPi - g[6]);
        r[0] = r[0] * fx;
        r[6] = keep_w * r[6] + flip_w * (sgn(r[6]) * kPi - r[6]);
    }
    // canonical transformation
    const float cosr = cosf(r[6]), sinr = sinf(r[6]);
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
        if (a.aug) {
            rot_y(px, pz, ca, sa);
            px = px * sc; py = py * sc; pz = pz * sc;
            px = px * fx;
        }
        float dx = px - r[0], dz = pz - r[2];
        const float dy = py - r[1];
        rot_y(dx, dz, cosr, sinr);
        ox[s * 3 + 0] = dx; ox[s * 3 + 1] = dy; ox[s * 3 + 2] = dz;
        op[s] = dx; op[S + s] = dy; op[2 * S + s] = dz;
        op[3 * S + s] = mv;
        if (E > 1) op[4 * S + s] = dv;
    }
    if (a.C > 0) gather_rows(a.C, N, S, empty ? nullptr : feat + (int64_t)b * a.C * N, sidx, ofeat + (int64_t)bm * a.C * S);
    if (tid == 0) {
        const float roi_ry = py_mod(r[6], kTwoPi);
        float gx = g[0] - r[0], gz = g[2] - r[2];
        const float gy = g[1] - r[1], gry = g[6] - roi_ry;
        rot_y(gx, gz, cosf(roi_ry), sinf(roi_ry));
        float* og = ogt + (int64_t)bm * 7;
        og[0] = gx; og[1] = gy; og[2] = gz; og[3] = g[3]; og[4] = g[4]; og[5] = g[5]; og[6] = gry;
#pragma unroll
        for (int k = 0; k < 7; ++k) oroi[(int64_t)bm * 7 + k] = r[k];
        empty_flag[bm] = empty ? 1 : 0;
        const float iou = ious[bm];
        const bool no_cand = counts[(int64_t)b * kCounts + 4] != 0;
        int64_t cls = iou > a.cls_fg ? 1 : 0;
        if (empty || (iou > a.cls_bg && iou < a.cls_fg) || no_cand) cls = -1;
        cls_label[bm] = cls;
        reg_valid[bm] = (iou > a.reg_fg && !empty && !no_cand) ? 1 : 0;
    }
}

}  // namespace

extern "C" int drc_rcnn_sample_max_candidates(void) { return kMaxCand; }
extern "C" int drc_rcnn_sample_max_slots(void) { return kMaxSlots; }

extern "C" int drc_rcnn_sample_rois(int B, int M, int N, int P, int T, int fg_per_image, int method, float fg_thresh, float bg_thresh,
                                    float bg_thresh_lo, double hard_bg_ratio, const float* cand, const float* gt, const float* draws,
                                    int64_t draw_stride, float* rois, float* gt_of_rois, float* roi_iou, int32_t* src_index, int32_t* n_iter,
                                    int32_t* counts, void* stream) {
    if (B < 0 || M < 1 || M > kMaxCand || N < 1 || P < 1 || P > kMaxSlots || T < 0 || fg_per_image < 0 || fg_per_image > P) return -2;
    if (method != 0 && method != 1) return -2;
    if (!(hard_bg_ratio >= 0.0 && hard_bg_ratio <= 1.0)) return -2;
    if (draw_stride < (int64_t)M + P + (int64_t)P * T * 9 + (int64_t)P * 3) return -2;
    if (B == 0) return 0;
    if (!cand || !gt || !draws || !rois || !gt_of_rois || !roi_iou || !src_index || !n_iter || !counts) return -1;
    const SampleArgs a = {M, N, P, T, fg_per_image, method, fg_thresh, bg_thresh, bg_thresh_lo, hard_bg_ratio, draw_stride};
    hipLaunchKernelGGL(sample_rois_kernel, dim3((unsigned)B), dim3(kSampleThreads), 0, (hipStream_t)stream, a, cand, gt, draws, rois,
                       gt_of_rois, roi_iou, src_index, n_iter, counts);
    return (int)hipGetLastError();
}

extern "C" int drc_rcnn_pool_target_fwd(int B, int N, int P, int C, int S, const float* rpn_xyz, const float* feat, const float* seg_mask,
                                        const float* pts_depth, int use_depth, const float* rois, const float* gt_of_rois,
                                        const float* roi_iou, const int32_t* counts, const float* aug_draws, int64_t draw_stride, int aug,
                                        float rot_range, float extra_width, float extra_width2, float reg_fg_thresh, float cls_fg_thresh,
                                        float cls_bg_thresh, float* xyz, float* pts, float* ofeat, int32_t* empty_flag, float* roi_boxes3d,
                                        float* gt_ct, int64_t* cls_label, int64_t* reg_valid_mask, void* stream) {
    if (B < 0 || N < 0 || P < 0 || C < 0 || S < 1 || S > kMaxPoolSamples) return -2;
    if (aug && draw_stride < (int64_t)P * 3) return -2;
    const int64_t blocks = (int64_t)B * P;
    if (blocks == 0) return 0;
    if (blocks > INT32_MAX) return -2;
    if (!rois || !gt_of_rois || !roi_iou || !counts || (aug && !aug_draws)) return -1;
    if ((N > 0 && (!rpn_xyz || !seg_mask || (use_depth && !pts_depth))) || (N > 0 && C > 0 && !feat)) return -1;
    if (!xyz || !pts || (C > 0 && !ofeat) || !empty_flag || !roi_boxes3d || !gt_ct || !cls_label || !reg_valid_mask) return -1;
    const PoolTargetArgs a = {N, P, C, S, use_depth ? 2 : 1, aug ? 1 : 0, extra_width, extra_width2, rot_range, reg_fg_thresh,
                              cls_fg_thresh, cls_bg_thresh, draw_stride};
    hipLaunchKernelGGL(pool_target_kernel, dim3((unsigned)blocks), dim3(kPoolThreads), (size_t)((S + 3) & ~3) * sizeof(int32_t),
                       (hipStream_t)stream, a, rpn_xyz, feat, seg_mask, pts_depth, rois, gt_of_rois, roi_iou, counts, aug_draws, xyz, pts,
                       ofeat, empty_flag, roi_boxes3d, gt_ct, cls_label, reg_valid_mask);
    return (int)hipGetLastError();
}

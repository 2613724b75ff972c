// boxes3d.hip -- PointRCNN's 3D box ops (gfx950): rotated BEV overlap / IoU, fused 3D IoU, batched rotated and axis-aligned NMS,
// roipool3d and the per-point in-box flags.
//
//   reference: point_rcnn/lib/utils/iou3d/src/iou3d_kernel.cu (box_overlap, iou_bev, iou_normal, nms_kernel, nms_normal_kernel),
//              iou3d_utils.py (boxes_iou3d_gpu), roipool3d/src/roipool3d_kernel.cu (pt_in_box3d, get_pooled_idx, roipool3d_forward).
//
// Every value is the reference's fp32 expression, evaluated in the same order (the library builds with -ffp-contract=off).  The
// schedules are ours:
//   - a box's centre, rotated corners and trigonometry are computed once per box (rows: once per LDS tile, columns: once per lane),
//     not once per pair;
//   - the <= 24-point intersection polygon lives in registers: each candidate, in the reference's append order, lands in its
//     compacted slot through a select over the slots it can reach, then a stable insertion sort orders it as the reference's
//     bubble sort does; loops stop once no lane of the wave needs more.  No runtime-indexed private array, so no scratch;
//   - NMS: one wave per 64x64 tile, the lane is the column and __ballot gives each row's 64-bit word; tiles below the diagonal
//     (never read by the walk) are skipped.  The greedy walk runs on the device, one wave per batch row, the removal words spread
//     over the lanes (8 per lane: n <= 32768), and stops at max_keep;
//   - roipool3d: one workgroup per (batch, box) scans the points in index order, a ballot + popcount prefix places the first S
//     in-box indices in LDS, then whole output rows are gathered with coalesced stores.  No B*N*M assignment buffer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_pts.h"
#include "box3d_iou.h"
#include "box3d_pt.h"

namespace {

constexpr int kWalkSlots = 8;               // removal words per lane in the walk
constexpr int kMaxNmsBoxes = 64 * 64 * kWalkSlots;
using box3d_pt::kMaxPoolSamples;
using box3d_pt::kPoolThreads;
using box3d_pt::pt_in_box3d;                // shared with rcnn_ops.hip

using namespace box3d_iou;                  // BoxG, box_geom*, box_overlap, iou3d_of_overlap: shared with proposal_target.hip

__device__ __forceinline__ float iou_bev(const BoxG& A, const BoxG& B) {
    const float s = box_overlap(A, B);
    return s / fmaxf(A.area + B.area - s, kEps);
}

__device__ __forceinline__ float iou_normal(const BoxG& a, const BoxG& b) {
    const float left = fmaxf(a.x1, b.x1), right = fminf(a.x2, b.x2);
    const float top = fmaxf(a.y1, b.y1), bottom = fminf(a.y2, b.y2);
    const float width = fmaxf(right - left, 0.f), height = fmaxf(bottom - top, 0.f);
    const float inter = width * height;
    return inter / fmaxf(a.area + b.area - inter, kEps);
}

// ---- pairwise [Na, Nb]: 64 columns (one per lane) x 64 rows (16 per wave, geometry in LDS) per workgroup
enum { kOverlap = 0, kIou = 1, kIou3d = 2 };

template <int kMode>
__global__ __launch_bounds__(256) void pairwise_kernel(int Na, int Nb, const float* __restrict__ a, const float* __restrict__ b,
                                                       float* __restrict__ out) {
    constexpr int W = kMode == kIou3d ? 7 : 5;
    __shared__ BoxG ra[64];
    __shared__ float rh[64][3];             // 3D: y - h, y, h * w * l
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a0 = blockIdx.y * 64, bi = blockIdx.x * 64 + lane;
    if (tid < 64) {
        const float* p = a + (int64_t)min(a0 + tid, Na - 1) * W;
        ra[tid] = kMode == kIou3d ? box_geom7(p) : box_geom5(p);
        if (kMode == kIou3d) { rh[tid][0] = p[1] - p[3]; rh[tid][1] = p[1]; rh[tid][2] = p[3] * p[4] * p[5]; }
    }
    const float* q = b + (int64_t)min(bi, Nb - 1) * W;
    const BoxG cg = kMode == kIou3d ? box_geom7(q) : box_geom5(q);
    float bmin = 0.f, bmax = 0.f, bvol = 0.f;
    if (kMode == kIou3d) { bmin = q[1] - q[3]; bmax = q[1]; bvol = q[3] * q[4] * q[5]; }
    __syncthreads();
    for (int r = wave * 16; r < wave * 16 + 16; ++r) {
        const int ai = a0 + r;
        if (ai >= Na) break;                // uniform over the wave
        float v;
        if (kMode == kOverlap) {
            v = box_overlap(ra[r], cg);
        } else if (kMode == kIou) {
            v = iou_bev(ra[r], cg);
        } else {                            // boxes_iou3d_gpu after the BEV overlap, in its torch order
            v = iou3d_of_overlap(box_overlap(ra[r], cg), rh[r][0], rh[r][1], rh[r][2], bmin, bmax, bvol);
        }
        if (bi < Nb) out[(int64_t)ai * Nb + bi] = v;
    }
}

// ---- NMS suppression mask of every batch row: mask[b, i, c] bit t = box c*64+t (> i) overlaps box i by more than thresh
template <bool kNormal>
__global__ __launch_bounds__(64) void nms_mask_kernel(int Nmax, int cw, const float* __restrict__ boxes, const int32_t* __restrict__ counts,
                                                      float thresh, uint64_t* __restrict__ mask) {
    const int cb = blockIdx.x, rb = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
    if (cb < rb) return;                    // below the diagonal: never read
    const int n = min(max(counts[b], 0), Nmax);
    const int row0 = rb * 64, col0 = cb * 64;
    if (col0 >= n) return;
    const int rows = min(64, n - row0), cols = min(64, n - col0);
    const float* bb = boxes + (int64_t)b * Nmax * 5;
    __shared__ BoxG rg[64];
    if (lane < rows) rg[lane] = box_geom5(bb + (int64_t)(row0 + lane) * 5);
    const BoxG cg = box_geom5(bb + (int64_t)(col0 + min(lane, cols - 1)) * 5);
    __syncthreads();
    const bool diag = cb == rb;
    uint64_t word = 0;
    for (int r = 0; r < rows; ++r) {
        const bool live = lane < cols && (!diag || lane > r);
        const float v = kNormal ? iou_normal(rg[r], cg) : iou_bev(rg[r], cg);
        const uint64_t bal = __ballot(live && v > thresh);
        if (lane == r) word = bal;
    }
    if (lane < rows) mask[((int64_t)b * Nmax + row0 + lane) * cw + cb] = word;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}

// ---- the greedy walk of iou3d.cpp's nms_gpu, one wave per batch row: keep[b, k] = k-th kept position, num_keep[b]
__global__ __launch_bounds__(64) void nms_walk_kernel(int Nmax, int cw, const int32_t* __restrict__ counts, const uint64_t* __restrict__ mask,
                                                      int max_keep, int64_t* __restrict__ keep, int keep_stride, int32_t* __restrict__ num_keep) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = min(max(counts[b], 0), Nmax);
    const int cwn = (n + 63) / 64;
    const int lim = max_keep > 0 ? max_keep : n;
    const uint64_t* mb = mask + (int64_t)b * Nmax * cw;
    int64_t* kb = keep + (int64_t)b * keep_stride;
    uint64_t remv[kWalkSlots];
#pragma unroll
    for (int k = 0; k < kWalkSlots; ++k) remv[k] = 0;
    int kept = 0;
    for (int c = 0; c < cwn && kept < lim; ++c) {
        uint64_t mine = 0;
#pragma unroll
        for (int k = 0; k < kWalkSlots; ++k)
            if (k == (c >> 6)) mine = remv[k];
        uint64_t cur = shfl64(mine, c & 63);
        const int nb = min(64, n - c * 64);
        const uint64_t valid = nb == 64 ? ~0ull : ((1ull << nb) - 1ull);
        uint64_t todo = ~cur & valid;
        while (todo && kept < lim) {
            const int bit = __ffsll((unsigned long long)todo) - 1;
            const int i = c * 64 + bit;
            if (lane == 0) kb[kept] = i;
            ++kept;
            const uint64_t* row = mb + (int64_t)i * cw;
#pragma unroll
            for (int k = 0; k < kWalkSlots; ++k) {
                const int j = lane + 64 * k;
                if (j >= c && j < cwn) remv[k] |= row[j];
            }
            cur |= row[c];
            todo = ~cur & valid & ~((2ull << bit) - 1ull);     // bit 63: 2ull << 63 == 0, nothing left in this word
        }
    }
    if (lane == 0) num_keep[b] = kept;
}

// ---- roipool3d (pt_in_box3d and the selection of the first S in-box points: box3d_pt.h)
__global__ __launch_bounds__(kPoolThreads) void roipool3d_kernel(int N, int M, int C, int S, const float* __restrict__ xyz,
                                                                 const float* __restrict__ boxes3d, const float* __restrict__ feat,
                                                                 float* __restrict__ pooled, int32_t* __restrict__ empty_flag) {
    __shared__ int32_t sidx[kMaxPoolSamples];
    __shared__ int wcnt[kPoolThreads / 64];
    const int bm = blockIdx.x, b = bm / M;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* bx = boxes3d + (int64_t)bm * 7;
    const float cosa = cosf(bx[6]), sina = sinf(bx[6]);
    const float* p = xyz + (int64_t)b * N * 3;
    const int cnt = box3d_pt::select_in_box(N, S, p, bx, cosa, sina, sidx, wcnt);      // block-uniform
    if (cnt == 0) {
        if (tid == 0) empty_flag[bm] = 1;
        return;
    }
    const int have = min(cnt, S);
    const int row = 3 + C;
    const float* fb = feat + (int64_t)b * N * C;
    float* ob = pooled + (int64_t)bm * S * row;
    for (int s = wave; s < S; s += kPoolThreads / 64) {
        const int src = sidx[s % have];
        float* o = ob + (int64_t)s * row;
        for (int j = lane; j < row; j += 64)
            o[j] = j < 3 ? p[(int64_t)src * 3 + j] : fb[(int64_t)src * C + (j - 3)];
    }
}

__global__ __launch_bounds__(256) void pts_in_boxes3d_kernel(int N, int M, const float* __restrict__ xyz, const float* __restrict__ boxes3d,
                                                             uint8_t* __restrict__ flags) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int m = blockIdx.y, b = blockIdx.z;
    if (k >= N) return;
    const float* bx = boxes3d + ((int64_t)b * M + m) * 7;
    const float* q = xyz + ((int64_t)b * N + k) * 3;
    flags[((int64_t)b * M + m) * N + k] = pt_in_box3d(q[0], q[1], q[2], bx, cosf(bx[6]), sinf(bx[6])) ? 1 : 0;
}

template <int kMode>
int launch_pairwise(int Na, int Nb, const float* a, const float* b, float* out, void* stream) {
    if (Na < 0 || Nb < 0) return -2;
    if (Na == 0 || Nb == 0) return 0;
    if (!a || !b || !out) return -1;
    const int64_t gy = ((int64_t)Na + 63) / 64, gx = ((int64_t)Nb + 63) / 64;
    if (gy > 65535 || gx > INT32_MAX) return -2;
    hipLaunchKernelGGL(pairwise_kernel<kMode>, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, Na, Nb, a, b, out);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int drc_box3d_bev(int Na, int Nb, const float* a, const float* b, int mode, float* out, void* stream) {
    if (mode == 0) return launch_pairwise<kOverlap>(Na, Nb, a, b, out, stream);
    if (mode == 1) return launch_pairwise<kIou>(Na, Nb, a, b, out, stream);
    return -2;
}

extern "C" int drc_box3d_iou3d(int Na, int Nb, const float* a, const float* b, float* out, void* stream) {
    return launch_pairwise<kIou3d>(Na, Nb, a, b, out, stream);
}

extern "C" int drc_box3d_nms(int B, int Nmax, const float* boxes, const int32_t* counts, float thresh, int normal, int max_keep, uint64_t* mask,
                             int64_t* keep, int keep_stride, int32_t* num_keep, void* stream) {
    if (B < 0 || Nmax < 0 || Nmax > kMaxNmsBoxes || B > 65535) return -2;
    const int kmax = max_keep > 0 && max_keep < Nmax ? max_keep : Nmax;
    if (keep_stride < kmax) return -2;
    if (B == 0) return 0;
    if (!counts || !num_keep || (Nmax > 0 && (!boxes || !mask || !keep))) return -1;
    const int cw = (Nmax + 63) / 64;
    hipStream_t st = (hipStream_t)stream;
    if (Nmax > 0) {
        const dim3 grid((unsigned)cw, (unsigned)cw, (unsigned)B);
        if (normal)
            hipLaunchKernelGGL(nms_mask_kernel<true>, grid, dim3(64), 0, st, Nmax, cw, boxes, counts, thresh, mask);
        else
            hipLaunchKernelGGL(nms_mask_kernel<false>, grid, dim3(64), 0, st, Nmax, cw, boxes, counts, thresh, mask);
    }
    hipLaunchKernelGGL(nms_walk_kernel, dim3((unsigned)B), dim3(64), 0, st, Nmax, cw, counts, mask, max_keep, keep, keep_stride, num_keep);
    return (int)hipGetLastError();
}

extern "C" int drc_roipool3d_fwd(int B, int N, int M, int C, int S, const float* xyz, const float* boxes3d, const float* feat, float* pooled,
                                 int32_t* empty_flag, void* stream) {
    if (B < 0 || N < 0 || M < 0 || C < 0 || S < 0 || S > kMaxPoolSamples) return -2;
    const int64_t blocks = (int64_t)B * M;
    if (blocks == 0) return 0;
    if (blocks > INT32_MAX) return -2;
    if (!boxes3d || !empty_flag || (N > 0 && !xyz) || (N > 0 && C > 0 && !feat) || (S > 0 && !pooled)) return -1;
    hipLaunchKernelGGL(roipool3d_kernel, dim3((unsigned)blocks), dim3(kPoolThreads), 0, (hipStream_t)stream, N, M, C, S, xyz, boxes3d, feat,
                       pooled, empty_flag);
    return (int)hipGetLastError();
}

extern "C" int drc_pts_in_boxes3d(int B, int N, int M, const float* xyz, const float* boxes3d, uint8_t* flags, void* stream) {
    if (B < 0 || N < 0 || M < 0 || B > 65535 || M > 65535) return -2;
    if ((int64_t)B * M * N == 0) return 0;
    if (!xyz || !boxes3d || !flags) return -1;
    hipLaunchKernelGGL(pts_in_boxes3d_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)M, (unsigned)B), dim3(256), 0, (hipStream_t)stream, N,
                       M, xyz, boxes3d, flags);
    return (int)hipGetLastError();
}

extern "C" int drc_box3d_max_pool_samples(void) { return kMaxPoolSamples; }

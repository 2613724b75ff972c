// kitti_eval.hip -- the KITTI object benchmark's scoring (devkit evaluate_object.cpp: 2D, AOS, BEV and 3D average precision) on gfx950.
//
// The devkit recomputes every box overlap once per recall threshold, difficulty and frame.  Here the overlaps of every (ground truth,
// detection) pair of a frame are computed ONCE (overlaps_kernel) and every pass of the greedy assignment reads them:
//
//   clean_kernel     cleanData: per difficulty, the ignore code of every ground-truth row and detection
//   overlaps_kernel  one thread per pair: image IoU, rotated BEV IoU, 3D IoU (DontCare rows: criterion 0, over the detection's own size)
//   pass_kernel<0>   computeStatistics(compute_fp = false): one thread per (frame, difficulty, metric) -> the matched scores
//   pass_kernel<1>   computeStatistics(compute_fp = true):  one thread per (frame, difficulty, metric, threshold) -> tp, fp, fn, similarity
//   reduce_kernel    the sums over the frames, one workgroup per (difficulty, metric, threshold), in a fixed order: bit-identical run to run
//
// Everything is fp64 as in the devkit (the library builds with -ffp-contract=off), so `overlap > MIN_OVERLAP` falls as it does there.
// The input is ragged: frame f owns ground-truth rows gt_off[f] .. gt_off[f+1], detections det_off[f] .. det_off[f+1] and the pairs
// pair_off[f] + g * D_f + d.  The set of assigned detections of a frame is a bit mask of kMaxDet bits held in LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_pts.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxDet = 256;                 // detections of one frame (the assigned set: kMaxDet / 64 words)
constexpr int kMaxGt = 4096;                 // ground-truth rows of one frame
constexpr int kWords = kMaxDet / 64;
constexpr int kT = 41;                       // N_SAMPLE_PTS
constexpr int kGtCols = 14;                  // truncation, occlusion, alpha, x1, y1, x2, y2, h, w, l, t1, t2, t3, ry
constexpr int kDetCols = 13;                 // alpha, x1, y1, x2, y2, h, w, l, t1, t2, t3, ry, score
// class codes the host resolves (case-insensitively) for the class under evaluation
constexpr int kGtSelf = 0, kGtNeighbour = 1, kGtDontCare = 2;       // anything else: another class
constexpr int kDetSelf = 0;

__constant__ const int kMinHeight[3] = {40, 25, 25};
__constant__ const int kMaxOcclusion[3] = {0, 1, 2};
__constant__ const double kMaxTruncation[3] = {0.15, 0.3, 0.5};

// ---- cleanData ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void clean_kernel(int NG, int ND, const double* __restrict__ gt, const int32_t* __restrict__ gt_cls,
                                                         const double* __restrict__ det, const int32_t* __restrict__ det_cls,
                                                         int8_t* __restrict__ gt_ign, int8_t* __restrict__ det_ign) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < NG) {
        const double* g = gt + (int64_t)i * kGtCols;
        const double height = g[6] - g[4];
        const int occ = (int)g[1];
        const int c = gt_cls[i];
        for (int d = 0; d < 3; ++d) {
            // the evaluator ignores a ground truth of exactly the minimum height (<=), but keeps such a detection (<, below)
            const bool ignore = occ > kMaxOcclusion[d] || g[0] > kMaxTruncation[d] || height <= kMinHeight[d];
            int8_t v;
            if (c == kGtSelf && !ignore) v = 0;
            else if (c == kGtNeighbour || (ignore && c == kGtSelf)) v = 1;
            else v = -1;
            gt_ign[(int64_t)d * NG + i] = v;
        }
    } else if (i - NG < ND) {
        const int j = i - NG;
        const double* p = det + (int64_t)j * kDetCols;
        const int height = (int)fabs(p[2] - p[4]);          // the devkit keeps this one in an int32_t
        const int c = det_cls[j];
        for (int d = 0; d < 3; ++d) {
            int8_t v;
            if (height < kMinHeight[d]) v = 1;
            else if (c == kDetSelf) v = 0;
            else v = -1;
            det_ign[(int64_t)d * ND + j] = v;
        }
    }
}

// ---- overlaps ------------------------------------------------------------------------------------------------------------------------
// criterion -1: over the union; 0: over the detection's own area (a = detection)
__device__ __forceinline__ double image_overlap(const double* a, const double* b, bool over_a) {
    const double x1 = fmax(a[1], b[1]), y1 = fmax(a[2], b[2]), x2 = fmin(a[3], b[3]), y2 = fmin(a[4], b[4]);
    const double w = x2 - x1, h = y2 - y1;
    if (w <= 0 || h <= 0) return 0;
    const double inter = w * h;
    const double a_area = (a[3] - a[1]) * (a[4] - a[2]);
    const double b_area = (b[3] - b[1]) * (b[4] - b[2]);
    return over_a ? inter / a_area : inter / (a_area + b_area - inter);
}

struct Rect {
    double cx, cz, l, w, ry;
};

// clip the polygon against the half plane s * coordinate(axis) <= lim.  A quadrilateral clipped four times has at most 8 vertices; the
// arrays hold kMaxVerts and the writes are bounded all the same.
constexpr int kMaxVerts = 12;
__device__ __forceinline__ int clip_axis(const double* px, const double* py, int n, double* qx, double* qy, int axis, double s, double lim) {
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const int k = (i + 1 == n) ? 0 : i + 1;
        const double ax = px[i], ay = py[i], bx = px[k], by = py[k];
        const double da = s * (axis ? ay : ax) - lim, db = s * (axis ? by : bx) - lim;
        const bool ina = da <= 0, inb = db <= 0;
        if (ina && m < kMaxVerts) { qx[m] = ax; qy[m] = ay; ++m; }
        if (ina != inb && m < kMaxVerts) {
            const double t = da / (da - db);
            qx[m] = ax + t * (bx - ax); qy[m] = ay + t * (by - ay); ++m;
        }
    }
    return m;
}

// area of the intersection of two rotated rectangles: a's corners in b's own frame, clipped to b's extents, then the shoelace formula
__device__ double bev_intersection(const Rect& a, const Rect& b) {
    double px[kMaxVerts], py[kMaxVerts], qx[kMaxVerts], qy[kMaxVerts];
    const double ca = cos(a.ry), sa = sin(a.ry), cb = cos(b.ry), sb = sin(b.ry);
    const double hl = a.l / 2, hw = a.w / 2;
    const double lx[4] = {hl, hl, -hl, -hl}, lz[4] = {hw, -hw, -hw, hw};
    for (int i = 0; i < 4; ++i) {
        // the devkit's toPolygon: [cos sin; -sin cos] * corner + (t1, t3)
        const double wx = (ca * lx[i] + sa * lz[i]) + a.cx - b.cx;
        const double wz = ((-sa) * lx[i] + ca * lz[i]) + a.cz - b.cz;
        px[i] = cb * wx + (-sb) * wz;                       // the inverse of b's rotation
        py[i] = sb * wx + cb * wz;
    }
    const double bl = fabs(b.l) / 2, bw = fabs(b.w) / 2;
    int n = clip_axis(px, py, 4, qx, qy, 0, 1.0, bl);
    n = clip_axis(qx, qy, n, px, py, 0, -1.0, bl);
    n = clip_axis(px, py, n, qx, qy, 1, 1.0, bw);
    n = clip_axis(qx, qy, n, px, py, 1, -1.0, bw);
    if (n < 3) return 0;
    double s = 0;
    for (int i = 0; i < n; ++i) {
        const int k = (i + 1 == n) ? 0 : i + 1;
        s += px[i] * py[k] - px[k] * py[i];
    }
    return fabs(s) / 2;
}

__global__ __launch_bounds__(kThreads) void overlaps_kernel(int F, int64_t NP, const double* __restrict__ gt, const int32_t* __restrict__ gt_cls,
                                                            const double* __restrict__ det, const int32_t* __restrict__ gt_off,
                                                            const int32_t* __restrict__ det_off, const int64_t* __restrict__ pair_off,
                                                            int metric_mask, double* __restrict__ ov) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= NP) return;
    int lo = 0, hi = F;                                     // the frame: the last f with pair_off[f] <= p
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pair_off[mid] <= p) lo = mid; else hi = mid;
    }
    const int f = lo;
    const int D = det_off[f + 1] - det_off[f];
    const int64_t r = p - pair_off[f];
    const int gi = gt_off[f] + (int)(r / D), di = det_off[f] + (int)(r % D);
    const double* g = gt + (int64_t)gi * kGtCols + 2;       // alpha, x1, y1, x2, y2, h, w, l, t1, t2, t3, ry
    const double* d = det + (int64_t)di * kDetCols;
    const bool over_det = gt_cls[gi] == kGtDontCare;
    if (metric_mask & 1) ov[p] = image_overlap(d, g, over_det);
    if (metric_mask & 6) {
        const Rect rd = {d[8], d[10], d[7], d[6], d[11]}, rg = {g[8], g[10], g[7], g[6], g[11]};
        const double inter = bev_intersection(rd, rg);
        const double d_area = fabs(d[7] * d[6]), g_area = fabs(g[7] * g[6]);
        if (metric_mask & 2) ov[NP + p] = over_det ? inter / d_area : inter / (d_area + g_area - inter);
        if (metric_mask & 4) {
            const double ymax = fmin(d[9], g[9]), ymin = fmax(d[9] - d[5], g[9] - g[5]);
            const double inter_vol = inter * fmax(0.0, ymax - ymin);
            const double d_vol = d[5] * d[7] * d[6], g_vol = g[5] * g[7] * g[6];
            ov[2 * NP + p] = over_det ? inter_vol / d_vol : inter_vol / (d_vol + g_vol - inter_vol);
        }
    }
}

// ---- computeStatistics -----------------------------------------------------------------------------------------------------------------
// FP = false: thread (frame, difficulty, metric)            -> v / matched [3,3,NG]: the score recorded for a ground-truth row, if any
// FP = true:  thread (frame, difficulty, metric, threshold) -> counts [3,3,41,3,F] int16 (tp, fp, fn) and sim [3,3,41,F]; all of them written
template <bool FP>
__global__ __launch_bounds__(kThreads) void pass_kernel(int F, int NG, int ND, int64_t NP, const double* __restrict__ gt,
                                                        const int32_t* __restrict__ gt_cls, const double* __restrict__ det,
                                                        const int32_t* __restrict__ gt_off, const int32_t* __restrict__ det_off,
                                                        const int64_t* __restrict__ pair_off, const int8_t* __restrict__ gt_ign,
                                                        const int8_t* __restrict__ det_ign, const double* __restrict__ ov, int metric_mask,
                                                        double mo0, double mo1, double mo2, int compute_aos, const double* __restrict__ thr,
                                                        const int32_t* __restrict__ nthr, double* __restrict__ v, int8_t* __restrict__ matched,
                                                        int16_t* __restrict__ counts, double* __restrict__ sim) {
    __shared__ uint64_t s_assigned[kWords][kThreads];
    const int f = blockIdx.x * kThreads + threadIdx.x;
    const int combo = blockIdx.y;                           // (difficulty * 3 + metric) [* 41 + threshold]
    const int t = FP ? combo % kT : 0;
    const int dm = FP ? combo / kT : combo;
    const int diff = dm / 3, metric = dm % 3;
    if (f >= F) return;
    const int g0 = gt_off[f], G = gt_off[f + 1] - g0, d0 = det_off[f], D = det_off[f + 1] - d0;
    const bool live = ((metric_mask >> metric) & 1) && D <= kMaxDet && (!FP || t < nthr[dm]);
    if (FP && !live) {
        for (int k = 0; k < 3; ++k) counts[((int64_t)combo * 3 + k) * F + f] = 0;
        sim[(int64_t)combo * F + f] = 0;
        return;
    }
    if (!FP) {
        for (int g = 0; g < G; ++g) matched[(int64_t)dm * NG + g0 + g] = 0;
        if (!live) return;
    }
    for (int w = 0; w < kWords; ++w) s_assigned[w][threadIdx.x] = 0;
    const double min_ov = metric == 0 ? mo0 : (metric == 1 ? mo1 : mo2);
    const double thresh = FP ? thr[combo] : 0.0;
    const int8_t* gi = gt_ign + (int64_t)diff * NG + g0;
    const int8_t* di = det_ign + (int64_t)diff * ND + d0;
    const double* o = ov + (int64_t)metric * NP + pair_off[f];
    const double* dets = det + (int64_t)d0 * kDetCols;
    const bool aos = FP && compute_aos && metric == 0;
    int tp = 0, fp = 0, fn = 0;
    double similarity = 0;
    for (int g = 0; g < G; ++g) {
        const int ig = gi[g];
        if (ig == -1) continue;
        int det_idx = -1;
        double best = -10000000.0, max_overlap = 0;         // NO_DETECTION
        bool assigned_ignored = false;
        for (int d = 0; d < D; ++d) {
            const int id = di[d];
            if (id == -1) continue;
            if ((s_assigned[d >> 6][threadIdx.x] >> (d & 63)) & 1) continue;
            const double score = dets[d * kDetCols + 12];
            if (FP && score < thresh) continue;
            const double overlap = o[(int64_t)g * D + d];
            if (!(overlap > min_ov)) continue;
            if (!FP) {
                if (score > best) { det_idx = d; best = score; }
            } else if (id == 0) {
                if (overlap > max_overlap || assigned_ignored) { max_overlap = overlap; det_idx = d; assigned_ignored = false; }
            } else if (det_idx < 0) {
                det_idx = d; assigned_ignored = true;
            }
        }
        if (det_idx < 0) {
            if (ig == 0) ++fn;
            continue;
        }
        s_assigned[det_idx >> 6][threadIdx.x] |= 1ull << (det_idx & 63);
        if (ig == 1 || di[det_idx] == 1) continue;
        ++tp;
        if (!FP) {
            v[(int64_t)dm * NG + g0 + g] = dets[det_idx * kDetCols + 12];
            matched[(int64_t)dm * NG + g0 + g] = 1;
        }
        if (aos) similarity += (1.0 + cos(gt[(int64_t)(g0 + g) * kGtCols + 2] - dets[det_idx * kDetCols])) / 2.0;
    }
    if (!FP) return;
    for (int d = 0; d < D; ++d) {
        const bool as = (s_assigned[d >> 6][threadIdx.x] >> (d & 63)) & 1;
        if (!(as || di[d] != 0 || dets[d * kDetCols + 12] < thresh)) ++fp;
    }
    int nstuff = 0;
    for (int g = 0; g < G; ++g) {
        if (gt_cls[g0 + g] != kGtDontCare) continue;
        for (int d = 0; d < D; ++d) {
            if ((s_assigned[d >> 6][threadIdx.x] >> (d & 63)) & 1) continue;
            if (di[d] != 0) continue;
            if (dets[d * kDetCols + 12] < thresh) continue;
            if (o[(int64_t)g * D + d] > min_ov) {
                s_assigned[d >> 6][threadIdx.x] |= 1ull << (d & 63);
                ++nstuff;
            }
        }
    }
    fp -= nstuff;
    counts[((int64_t)combo * 3 + 0) * F + f] = (int16_t)tp;              // at most kMaxGt = 4096 each: 16 bits hold them
    counts[((int64_t)combo * 3 + 1) * F + f] = (int16_t)fp;
    counts[((int64_t)combo * 3 + 2) * F + f] = (int16_t)fn;
    sim[(int64_t)combo * F + f] = (aos && (tp > 0 || fp > 0)) ? similarity : 0.0;   // the devkit's -1 ("skip this frame") adds nothing
}

// ---- the sums over the frames -------------------------------------------------------------------------------------------------------------
// One workgroup per (difficulty, metric, threshold): thread i sums frames i, i + 256, ... in that order, then a tree over the 256 partial
// sums.  The order depends on F alone.
__global__ __launch_bounds__(kThreads) void reduce_kernel(int F, const int16_t* __restrict__ counts, const double* __restrict__ sim,
                                                          int64_t* __restrict__ out_counts, double* __restrict__ out_sim) {
    __shared__ int64_t s_c[3][kThreads];
    __shared__ double s_s[kThreads];
    const int combo = blockIdx.x, i = threadIdx.x;
    int64_t c[3] = {0, 0, 0};
    double s = 0;
    for (int f = i; f < F; f += kThreads) {
        for (int k = 0; k < 3; ++k) c[k] += counts[((int64_t)combo * 3 + k) * F + f];
        s += sim[(int64_t)combo * F + f];
    }
    for (int k = 0; k < 3; ++k) s_c[k][i] = c[k];
    s_s[i] = s;
    __syncthreads();
    for (int step = kThreads / 2; step > 0; step >>= 1) {
        if (i < step) {
            for (int k = 0; k < 3; ++k) s_c[k][i] += s_c[k][i + step];
            s_s[i] += s_s[i + step];
        }
        __syncthreads();
    }
    if (i == 0) {
        for (int k = 0; k < 3; ++k) out_counts[(int64_t)combo * 3 + k] = s_c[k][0];
        out_sim[combo] = s_s[0];
    }
}

__host__ int check_sizes(int F, int NG, int ND, int64_t NP, int max_gt, int max_det) {
    if (F < 0 || NG < 0 || ND < 0 || NP < 0 || max_gt < 0 || max_det < 0) return -2;
    if (max_gt > kMaxGt || max_det > kMaxDet) return -3;
    if ((int64_t)F * kT * 27 > INT32_MAX * 8LL || NP > (int64_t)INT32_MAX * kThreads) return -2;
    return 0;
}

}  // namespace

extern "C" int drc_kitti_eval_max_det(void) { return kMaxDet; }
extern "C" int drc_kitti_eval_max_gt(void) { return kMaxGt; }

extern "C" int drc_kitti_eval_clean(int NG, int ND, const double* gt, const int32_t* gt_cls, const double* det, const int32_t* det_cls,
                                    int8_t* gt_ign, int8_t* det_ign, void* stream) {
    if (NG < 0 || ND < 0) return -2;
    if (NG + (int64_t)ND == 0) return 0;
    if ((NG > 0 && (!gt || !gt_cls || !gt_ign)) || (ND > 0 && (!det || !det_cls || !det_ign))) return -1;
    if ((int64_t)NG + ND > INT32_MAX - kThreads) return -2;
    const unsigned blocks = (unsigned)(((int64_t)NG + ND + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(clean_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, NG, ND, gt, gt_cls, det, det_cls, gt_ign, det_ign);
    return (int)hipGetLastError();
}

extern "C" int drc_kitti_eval_overlaps(int F, int64_t NP, const double* gt, const int32_t* gt_cls, const double* det, const int32_t* gt_off,
                                       const int32_t* det_off, const int64_t* pair_off, int metric_mask, double* ov, void* stream) {
    if (F < 0 || NP < 0 || metric_mask < 0 || metric_mask > 7) return -2;
    if (F == 0 || NP == 0 || metric_mask == 0) return 0;
    if (!gt || !gt_cls || !det || !gt_off || !det_off || !pair_off || !ov) return -1;
    if (NP > (int64_t)INT32_MAX * kThreads) return -2;
    const unsigned blocks = (unsigned)((NP + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(overlaps_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, F, NP, gt, gt_cls, det, gt_off, det_off, pair_off,
                       metric_mask, ov);
    return (int)hipGetLastError();
}

extern "C" int drc_kitti_eval_pass1(int F, int NG, int ND, int64_t NP, int max_gt, int max_det, const double* gt, const int32_t* gt_cls,
                                    const double* det, const int32_t* gt_off, const int32_t* det_off, const int64_t* pair_off,
                                    const int8_t* gt_ign, const int8_t* det_ign, const double* ov, int metric_mask, double min_overlap_image,
                                    double min_overlap_ground, double min_overlap_3d, double* v, int8_t* matched, void* stream) {
    const int st = check_sizes(F, NG, ND, NP, max_gt, max_det);
    if (st) return st;
    if (metric_mask < 0 || metric_mask > 7) return -2;
    if (F == 0 || NG == 0) return 0;
    if (!gt || !gt_cls || !gt_off || !det_off || !pair_off || !gt_ign || !v || !matched) return -1;
    if (ND > 0 && NP > 0 && (!det || !det_ign || !ov)) return -1;
    const dim3 grid((unsigned)((F + kThreads - 1) / kThreads), 9u);
    hipLaunchKernelGGL(pass_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, F, NG, ND, NP, gt, gt_cls, det, gt_off, det_off, pair_off,
                       gt_ign, det_ign, ov, metric_mask, min_overlap_image, min_overlap_ground, min_overlap_3d, 0, (const double*)nullptr,
                       (const int32_t*)nullptr, v, matched, (int16_t*)nullptr, (double*)nullptr);
    return (int)hipGetLastError();
}

extern "C" int drc_kitti_eval_pass2(int F, int NG, int ND, int64_t NP, int max_gt, int max_det, const double* gt, const int32_t* gt_cls,
                                    const double* det, const int32_t* gt_off, const int32_t* det_off, const int64_t* pair_off,
                                    const int8_t* gt_ign, const int8_t* det_ign, const double* ov, int metric_mask, double min_overlap_image,
                                    double min_overlap_ground, double min_overlap_3d, int compute_aos, const double* thresholds,
                                    const int32_t* n_thresholds, int16_t* counts, double* sim, void* stream) {
    const int st = check_sizes(F, NG, ND, NP, max_gt, max_det);
    if (st) return st;
    if (metric_mask < 0 || metric_mask > 7) return -2;
    if (F == 0) return 0;
    if (!gt_off || !det_off || !pair_off || !thresholds || !n_thresholds || !counts || !sim) return -1;
    if (NG > 0 && (!gt || !gt_cls || !gt_ign)) return -1;
    if (ND > 0 && (!det || !det_ign)) return -1;
    if (NP > 0 && !ov) return -1;
    const dim3 grid((unsigned)((F + kThreads - 1) / kThreads), (unsigned)(9 * kT));
    hipLaunchKernelGGL(pass_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, F, NG, ND, NP, gt, gt_cls, det, gt_off, det_off, pair_off,
                       gt_ign, det_ign, ov, metric_mask, min_overlap_image, min_overlap_ground, min_overlap_3d, compute_aos, thresholds,
                       n_thresholds, (double*)nullptr, (int8_t*)nullptr, counts, sim);
    return (int)hipGetLastError();
}

extern "C" int drc_kitti_eval_reduce(int F, const int16_t* counts, const double* sim, int64_t* out_counts, double* out_sim, void* stream) {
    if (F < 0) return -2;
    if (!out_counts || !out_sim || (F > 0 && (!counts || !sim))) return -1;
    if ((int64_t)F * kT * 27 > INT32_MAX * 8LL) return -2;
    hipLaunchKernelGGL(reduce_kernel, dim3(9 * kT), dim3(kThreads), 0, (hipStream_t)stream, F, counts, sim, out_counts, out_sim);
    return (int)hipGetLastError();
}

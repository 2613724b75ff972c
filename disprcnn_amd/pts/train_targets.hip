// train_targets.hip -- PointRCNN's training labels and losses (gfx950): the RPN's per-point labels, the bin-based box regression loss
// and the three point classification losses, each with its gradient with respect to the network output.
//
//   reference: point_rcnn/lib/net/point_rcnn.py (generate_rpn_training_labels, filter_bbox_3d), utils/loss_utils.py (get_reg_loss,
//              DiceLoss, SigmoidFocalClassificationLoss), net/rpn_loss.py, net/rcnn_loss.py.
//
// What is fixed by the reference and what is ours:
//   - every LABEL (inside tests, bin indices, residual targets) is the reference's fp32 expression in its order (the library builds with
//     -ffp-contract=off; the Python doubles it mixes in arrive rounded to fp32 one at a time, as decode_rpn_boxes documents), so a row
//     lands in the reference's bin;
//   - every LOSS value is evaluated in fp64 from those fp32 labels and the fp32 predictions, summed in fp64, and rounded once.
// Schedule: the regression loss gives a wave to a row.  Lane c holds channel c (and c + 64), so a row is one coalesced read, each
// cross-entropy's logsumexp is a wave reduction over the lanes of its segment, and the label channel is a lane pick.  A wave keeps its
// sums in registers over its rows (row order), a block adds its 4 waves in wave order, and a one-block finish kernel adds the blocks'
// partials in block order: no atomics, two runs give the same bits.  Nothing here synchronises with the host or branches on a count:
// the reference's `if count != 0: divide` is a select on the device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_pts.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 1024;
constexpr int kSlots = 16;            // doubles per block partial (DRC_TRAIN_SCRATCH_DOUBLES = kMaxBlocks * kSlots)
constexpr int kRegSums = 11;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// torch.remainder(a, b) for b > 0: fmod, then the divisor's sign
__device__ __forceinline__ float t_remainder(float a, float b) {
    float r = fmodf(a, b);
    if (r != 0.f && r < 0.f) r = r + b;
    return r;
}
__device__ __forceinline__ float t_clamp(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }
__device__ __forceinline__ int bin_of(float q, int n) {
    int b = (int)floorf(q);
    return b < 0 ? 0 : (b >= n ? n - 1 : b);        // the reference's own ranges keep q inside [0, n); the clamp only guards memory
}

struct RegCfg {
    int C, P, YB, H, xz_fine, y_by_bin, ry_fine, anchor_per_row;
    float loc_scope, loc_clamp, loc_bin, loc_half_bin;
    float y_scope, y_clamp, y_bin, y_half_bin;
    float apc, half_apc, two_pi, pi, half_pi, three_half_pi, quarter_pi, ry_lo, ry_hi;
    // channel offsets
    int x_res, z_res, y_l, y_res, ry_l, ry_res, size_l;
};

struct RowT {
    int xb, zb, yb, rb;
    float xr, zr, yr, rr, sz[3];      // yr: the y offset label itself when y is not binned
};

__device__ __forceinline__ RowT row_targets(const float* __restrict__ lab, const float* __restrict__ anchor, const RegCfg& k) {
    RowT t;
    const float xs = t_clamp(lab[0] + k.loc_scope, 0.f, k.loc_clamp);
    const float zs = t_clamp(lab[2] + k.loc_scope, 0.f, k.loc_clamp);
    t.xb = bin_of(xs / k.loc_bin, k.P);
    t.zb = bin_of(zs / k.loc_bin, k.P);
    t.xr = (xs - ((float)t.xb * k.loc_bin + k.loc_half_bin)) / k.loc_bin;
    t.zr = (zs - ((float)t.zb * k.loc_bin + k.loc_half_bin)) / k.loc_bin;
    if (k.y_by_bin) {
        const float ys = t_clamp(lab[1] + k.y_scope, 0.f, k.y_clamp);
        t.yb = bin_of(ys / k.y_bin, k.YB);
        t.yr = (ys - ((float)t.yb * k.y_bin + k.y_half_bin)) / k.y_bin;
    } else {
        t.yb = -1;
        t.yr = lab[1];
    }
    float shift;
    if (k.ry_fine) {
        float r = t_remainder(lab[6], k.two_pi);
        if (r > k.half_pi && r < k.three_half_pi) r = t_remainder(r + k.pi, k.two_pi);
        shift = t_remainder(r + k.half_pi, k.two_pi);
        shift = t_clamp(shift - k.quarter_pi, k.ry_lo, k.ry_hi);
    } else {
        const float heading = t_remainder(lab[6], k.two_pi);
        shift = t_remainder(heading + k.half_apc, k.two_pi);
    }
    t.rb = bin_of(shift / k.apc, k.H);
    t.rr = (shift - ((float)t.rb * k.apc + k.half_apc)) / k.half_apc;
#pragma unroll
    for (int i = 0; i < 3; ++i) t.sz[i] = (lab[3 + i] - anchor[i]) / anchor[i];
    return t;
}

// ---- the wave's row: channel c lives in lane c & 63, slot c >> 6
struct RowV {
    float v0, v1;
};
__device__ __forceinline__ float pick(const RowV& r, int c) {
    const float a = __shfl(r.v0, c & 63), b = __shfl(r.v1, c & 63);
    return c < 64 ? a : b;
}
// value of this lane inside the segment [l, l + n), n <= 64: at most one of the lane's two channels is in it
__device__ __forceinline__ bool seg_val(const RowV& r, int lane, int l, int n, float& x, int& c) {
    const int c0 = lane, c1 = lane + 64;
    if (c0 >= l && c0 < l + n) { x = r.v0; c = c0; return true; }
    if (c1 >= l && c1 < l + n) { x = r.v1; c = c1; return true; }
    x = 0.f; c = -1;
    return false;
}
// max and sum of exp(x - max) over a segment
__device__ __forceinline__ void seg_stats(const RowV& r, int lane, int l, int n, float& mx, double& se) {
    float x; int c;
    const bool in = seg_val(r, lane, l, n, x, c);
    mx = wave_max(in ? x : -INFINITY);
    se = wave_sum(in ? exp((double)x - (double)mx) : 0.0);
}
__device__ __forceinline__ double smooth_l1(double d) {
    d = fabs(d);
    return d < 1.0 ? 0.5 * d * d : d - 0.5;
}
__device__ __forceinline__ double clamp1(double d) { return d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d); }

__global__ __launch_bounds__(kThreads) void reg_targets_kernel(const float* __restrict__ lab, const float* __restrict__ anchor, long rows,
                                                               RegCfg k, int32_t* __restrict__ bins, float* __restrict__ res) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= rows) return;
    const RowT t = row_targets(lab + i * 7, anchor + (k.anchor_per_row ? i * 3 : 0), k);
    bins[i * 4 + 0] = t.xb; bins[i * 4 + 1] = t.zb; bins[i * 4 + 2] = t.yb; bins[i * 4 + 3] = t.rb;
    res[i * 7 + 0] = t.xr; res[i * 7 + 1] = t.zr; res[i * 7 + 2] = t.yr; res[i * 7 + 3] = t.rr;
    res[i * 7 + 4] = t.sz[0]; res[i * 7 + 5] = t.sz[1]; res[i * 7 + 6] = t.sz[2];
}

// block partial [kSlots]: 0 x_bin, 1 z_bin, 2 x_res, 3 z_res, 4 y_offset | y_bin, 5 y_res, 6 ry_bin, 7 ry_res, 8 size, 9 selected rows,
// 10 selected rows with loss_mask (= 9 without one).  Sums 0-8 carry the loss_mask weight, except the binned y terms.
__global__ __launch_bounds__(kThreads) void reg_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ lab,
                                                           const uint8_t* __restrict__ row_mask, const uint8_t* __restrict__ loss_mask,
                                                           const float* __restrict__ anchor, long rows, RegCfg k, double* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[kRegSums];
#pragma unroll
    for (int i = 0; i < kRegSums; ++i) acc[i] = 0.0;
    for (long row = (long)blockIdx.x * kWaves + wave; row < rows; row += (long)gridDim.x * kWaves) {
        if (!row_mask[row]) continue;
        RowV r;
        r.v0 = lane < k.C ? pred[row * k.C + lane] : 0.f;
        r.v1 = lane + 64 < k.C ? pred[row * k.C + 64 + lane] : 0.f;
        const RowT t = row_targets(lab + row * 7, anchor + (k.anchor_per_row ? row * 3 : 0), k);
        const double w = loss_mask ? (loss_mask[row] ? 1.0 : 0.0) : 1.0;
        float mx; double se;
        seg_stats(r, lane, 0, k.P, mx, se);
        acc[0] += w * ((double)mx + log(se) - (double)pick(r, t.xb));
        seg_stats(r, lane, k.P, k.P, mx, se);
        acc[1] += w * ((double)mx + log(se) - (double)pick(r, k.P + t.zb));
        if (k.xz_fine) {
            acc[2] += w * smooth_l1((double)pick(r, k.x_res + t.xb) - (double)t.xr);
            acc[3] += w * smooth_l1((double)pick(r, k.z_res + t.zb) - (double)t.zr);
        }
        if (k.y_by_bin) {
            seg_stats(r, lane, k.y_l, k.YB, mx, se);
            acc[4] += (double)mx + log(se) - (double)pick(r, k.y_l + t.yb);
            acc[5] += smooth_l1((double)pick(r, k.y_res + t.yb) - (double)t.yr);
        } else {
            acc[4] += w * smooth_l1((double)pick(r, k.y_l) - (double)t.yr);
        }
        seg_stats(r, lane, k.ry_l, k.H, mx, se);
        acc[6] += w * ((double)mx + log(se) - (double)pick(r, k.ry_l + t.rb));
        acc[7] += w * smooth_l1((double)pick(r, k.ry_res + t.rb) - (double)t.rr);
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) s += smooth_l1((double)pick(r, k.size_l + i) - (double)t.sz[i]);
        acc[8] += w * s;
        acc[9] += 1.0;
        acc[10] += w;
    }
    __shared__ double red[kWaves][kRegSums];
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < kRegSums; ++i) red[wave][i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x < kSlots) {
        double v = 0.0;
        if (threadIdx.x < kRegSums)
            for (int wv = 0; wv < kWaves; ++wv) v += red[wv][threadIdx.x];
        part[(long)blockIdx.x * kSlots + threadIdx.x] = v;
    }
}

struct RegDenoms {
    double dm, dy, dsize;
};
__device__ __forceinline__ RegDenoms reg_denoms(double n_sel, double n_mask, int has_mask, int y_by_bin) {
    RegDenoms d;
    const double cnt = has_mask ? n_mask : n_sel;
    d.dm = cnt != 0.0 ? cnt : 1.0;                           // "if loss_mask.sum() != 0: divide"; a mean over no row is left a zero
    d.dsize = has_mask ? d.dm : 3.0 * d.dm;                  // 'none' + sum / count vs. 'mean' over rows x 3
    d.dy = y_by_bin ? (n_sel != 0.0 ? n_sel : 1.0) : d.dm;   // the binned y terms are plain means
    return d;
}

// sums[k] = partials added in block order (16 lanes per sum take blocks l, l + 16, ... in order, then a fixed xor tree), then the terms
// mode 0: regression.  terms [16]: 0-8 the normalised terms in the partial's order, 9 loss_loc, 10 loss_angle, 11 loss_size (= 8),
//         12 selected rows, 13 rows with loss_mask.
// mode 1-3: classification (BCE, focal, dice).  terms [8]: 0 loss, 1 positive part, 2 negative part (focal), 3 the normaliser before its
//         clamp (valid rows, positives, the union sum).
__global__ __launch_bounds__(kThreads) void finish_kernel(const double* __restrict__ part, int nblocks, int mode, int has_mask, int xz_fine,
                                                          int y_by_bin, double* __restrict__ sums, float* __restrict__ terms) {
    __shared__ double s[kSlots];
    const int k = threadIdx.x >> 4, l = threadIdx.x & 15;
    double v = 0.0;
    for (int i = l; i < nblocks; i += 16) v += part[(long)i * kSlots + k];
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    if (l == 0) { s[k] = v; sums[k] = v; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (mode == 0) {
        const RegDenoms d = reg_denoms(s[9], s[10], has_mask, y_by_bin);
        double t[9];
        for (int i = 0; i < 9; ++i) t[i] = s[i] / d.dm;
        t[8] = s[8] / d.dsize;
        if (y_by_bin) { t[4] = s[4] / d.dy; t[5] = s[5] / d.dy; }
        double loc = t[0] + t[1];
        if (xz_fine) loc += t[2] + t[3];
        loc += t[4];
        if (y_by_bin) loc += t[5];
        for (int i = 0; i < 9; ++i) terms[i] = (float)t[i];
        terms[9] = (float)loc;
        terms[10] = (float)(t[6] + t[7]);
        terms[11] = (float)t[8];
        terms[12] = (float)s[9];
        terms[13] = (float)s[10];
        terms[14] = 0.f; terms[15] = 0.f;
    } else if (mode == 1) {
        const double n = s[1] < 1.0 ? 1.0 : s[1];
        terms[0] = (float)(s[0] / n); terms[1] = 0.f; terms[2] = 0.f; terms[3] = (float)s[1];
        for (int i = 4; i < 8; ++i) terms[i] = 0.f;
    } else if (mode == 2) {
        const double n = s[2] < 1.0 ? 1.0 : s[2];
        terms[0] = (float)((s[0] + s[1]) / n); terms[1] = (float)(s[0] / n); terms[2] = (float)(s[1] / n); terms[3] = (float)s[2];
        for (int i = 4; i < 8; ++i) terms[i] = 0.f;
    } else {
        const double u = s[1] < 1.0 ? 1.0 : s[1];
        terms[0] = (float)(1.0 - s[0] / u); terms[1] = (float)s[0]; terms[2] = 0.f; terms[3] = (float)s[1];
        for (int i = 4; i < 8; ++i) terms[i] = 0.f;
    }
}

// d (g_loc * loss_loc + g_angle * loss_angle + g_size * loss_size) / d pred_reg, every element of grad written (zero on unselected rows)
__global__ __launch_bounds__(kThreads) void reg_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ lab,
                                                           const uint8_t* __restrict__ row_mask, const uint8_t* __restrict__ loss_mask,
                                                           const float* __restrict__ anchor, long rows, RegCfg k, const double* __restrict__ sums,
                                                           const float* __restrict__ g_loc, const float* __restrict__ g_angle,
                                                           const float* __restrict__ g_size, float* __restrict__ grad) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const RegDenoms d = reg_denoms(sums[9], sums[10], loss_mask != nullptr, k.y_by_bin);
    const double gl = g_loc ? (double)g_loc[0] : 0.0, ga = g_angle ? (double)g_angle[0] : 0.0, gs = g_size ? (double)g_size[0] : 0.0;
    for (long row = (long)blockIdx.x * kWaves + wave; row < rows; row += (long)gridDim.x * kWaves) {
        float* g = grad + row * k.C;
        if (!row_mask[row]) {
            if (lane < k.C) g[lane] = 0.f;
            if (lane + 64 < k.C) g[lane + 64] = 0.f;
            continue;
        }
        RowV r;
        r.v0 = lane < k.C ? pred[row * k.C + lane] : 0.f;
        r.v1 = lane + 64 < k.C ? pred[row * k.C + 64 + lane] : 0.f;
        const RowT t = row_targets(lab + row * 7, anchor + (k.anchor_per_row ? row * 3 : 0), k);
        const double w = loss_mask ? (loss_mask[row] ? 1.0 : 0.0) : 1.0;
        const double c_loc = gl * w / d.dm, c_y = k.y_by_bin ? gl / d.dy : c_loc, c_ang = ga * w / d.dm, c_size = gs * w / d.dsize;
        float mxx, mxz, mxy = 0.f, mxr;
        double sex, sez, sey = 1.0, ser;
        seg_stats(r, lane, 0, k.P, mxx, sex);
        seg_stats(r, lane, k.P, k.P, mxz, sez);
        if (k.y_by_bin) seg_stats(r, lane, k.y_l, k.YB, mxy, sey);
        seg_stats(r, lane, k.ry_l, k.H, mxr, ser);
#pragma unroll
        for (int slot = 0; slot < 2; ++slot) {
            const int c = lane + slot * 64;
            if (c >= k.C) continue;
            const double x = (double)(slot ? r.v1 : r.v0);
            double gv = 0.0;
            if (c < k.P) gv = c_loc * (exp(x - (double)mxx) / sex - (c == t.xb ? 1.0 : 0.0));
            else if (c < 2 * k.P) gv = c_loc * (exp(x - (double)mxz) / sez - (c - k.P == t.zb ? 1.0 : 0.0));
            else if (c < k.y_l) {            // the fine x / z residuals (only present with xz_fine)
                if (c == k.x_res + t.xb) gv = c_loc * clamp1(x - (double)t.xr);
                else if (c == k.z_res + t.zb) gv = c_loc * clamp1(x - (double)t.zr);
            } else if (c < k.ry_l) {
                if (!k.y_by_bin) gv = c_y * clamp1(x - (double)t.yr);
                else if (c < k.y_res) gv = c_y * (exp(x - (double)mxy) / sey - (c - k.y_l == t.yb ? 1.0 : 0.0));
                else if (c == k.y_res + t.yb) gv = c_y * clamp1(x - (double)t.yr);
            } else if (c < k.ry_res) gv = c_ang * (exp(x - (double)mxr) / ser - (c - k.ry_l == t.rb ? 1.0 : 0.0));
            else if (c < k.size_l) {
                if (c == k.ry_res + t.rb) gv = c_ang * clamp1(x - (double)t.rr);
            } else gv = c_size * clamp1(x - (double)t.sz[c - k.size_l]);
            g[c] = (float)gv;
        }
    }
}

// ---- classification losses, one thread per logit
struct ClsCfg {
    int kind;              // 1 BCE, 2 focal, 3 dice
    float fg_weight, alpha, gamma, ignore;
};
struct ClsRow {
    double a, b, c;        // the row's contribution to sums 0, 1, 2
};
__device__ __forceinline__ double sigmoid64(double x) { return x >= 0.0 ? 1.0 / (1.0 + exp(-x)) : exp(x) / (1.0 + exp(x)); }
__device__ __forceinline__ double bce_logits(double x, double t) { return fmax(x, 0.0) - x * t + log1p(exp(-fabs(x))); }

__device__ __forceinline__ ClsRow cls_row(float xf, float label, bool m, const ClsCfg& k) {
    ClsRow r = {0.0, 0.0, 0.0};
    const double x = (double)xf;
    if (k.kind == 1) {
        if (label >= 0.f && m) {
            const double t = label > 0.f ? 1.0 : 0.0;
            r.a = (label > 0.f ? (double)k.fg_weight : 1.0) * bce_logits(x, t);
            r.b = 1.0;
        }
    } else if (k.kind == 2) {
        if (m && (label > 0.f || label == 0.f)) {
            const double p = sigmoid64(x);
            if (label > 0.f) {
                r.a = pow(1.0 - p, (double)k.gamma) * (double)k.alpha * bce_logits(x, 1.0);
                r.c = 1.0;
            } else {
                r.b = pow(p, (double)k.gamma) * (1.0 - (double)k.alpha) * bce_logits(x, 0.0);
            }
        }
    } else {
        if (label != k.ignore) {
            const double p = sigmoid64(x), t = (double)label;
            r.a = fmin(p, t);
            r.b = fmax(p, t);
        }
    }
    return r;
}

__global__ __launch_bounds__(kThreads) void cls_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                           const uint8_t* __restrict__ mask, long n, ClsCfg k, double* __restrict__ part) {
    double a = 0.0, b = 0.0, c = 0.0;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
        const ClsRow r = cls_row(logits[i], labels[i], mask ? mask[i] != 0 : true, k);
        a += r.a; b += r.b; c += r.c;
    }
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
    __shared__ double red[kWaves][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave][0] = a; red[wave][1] = b; red[wave][2] = c; }
    __syncthreads();
    if (threadIdx.x < kSlots) {
        double v = 0.0;
        if (threadIdx.x < 3)
            for (int wv = 0; wv < kWaves; ++wv) v += red[wv][threadIdx.x];
        part[(long)blockIdx.x * kSlots + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(kThreads) void cls_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                           const uint8_t* __restrict__ mask, long n, ClsCfg k, const double* __restrict__ sums,
                                                           const float* __restrict__ gout, float* __restrict__ grad) {
    const double g = (double)gout[0];
    const double s0 = sums[0], s1 = sums[1], s2 = sums[2];
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
        const double x = (double)logits[i];
        const float label = labels[i];
        const bool m = mask ? mask[i] != 0 : true;
        const double p = sigmoid64(x);
        double gv = 0.0;
        if (k.kind == 1) {
            if (label >= 0.f && m) {
                const double t = label > 0.f ? 1.0 : 0.0;
                gv = (label > 0.f ? (double)k.fg_weight : 1.0) * (p - t) / (s1 < 1.0 ? 1.0 : s1);
            }
        } else if (k.kind == 2) {
            if (m && (label > 0.f || label == 0.f)) {
                const double nrm = s2 < 1.0 ? 1.0 : s2, gm = (double)k.gamma;
                if (label > 0.f) {
                    const double q = 1.0 - p;
                    gv = (double)k.alpha * pow(q, gm) * (-gm * p * bce_logits(x, 1.0) - q) / nrm;
                } else {
                    gv = (1.0 - (double)k.alpha) * pow(p, gm) * (gm * (1.0 - p) * bce_logits(x, 0.0) + p) / nrm;
                }
            }
        } else {
            if (label != k.ignore) {
                const double t = (double)label, dp = p * (1.0 - p), u = s1 < 1.0 ? 1.0 : s1;
                const double di = p < t ? dp : (p == t ? 0.5 * dp : 0.0);
                const double du = s1 >= 1.0 ? (p > t ? dp : (p == t ? 0.5 * dp : 0.0)) : 0.0;
                gv = -di / u + s0 * du / (u * u);
            }
        }
        grad[i] = (float)(g * gv);
    }
}

// SigmoidFocalClassificationLoss.forward, unreduced: out[i] = (1 - p_t)^gamma * alpha_t * ce(x, t) * weight[i] for any target t in [0, 1]
__device__ __forceinline__ void focal_elem(double x, double t, double alpha, double gm, double& f, double& df) {
    const double p = sigmoid64(x), ce = bce_logits(x, t);
    const double pt = t * p + (1.0 - t) * (1.0 - p), q = 1.0 - pt;
    const double aw = t * alpha + (1.0 - t) * (1.0 - alpha);
    const double mod = gm != 0.0 ? pow(q, gm) : 1.0;
    const double dmod = gm != 0.0 && q > 0.0 ? -gm * pow(q, gm - 1.0) * (2.0 * t - 1.0) * p * (1.0 - p) : 0.0;
    f = mod * aw * ce;
    df = aw * (dmod * ce + mod * (p - t));
}
__global__ __launch_bounds__(kThreads) void focal_elem_kernel(const float* __restrict__ logits, const float* __restrict__ targets,
                                                              const float* __restrict__ weights, long n, float alpha, float gamma,
                                                              const float* __restrict__ gout, float* __restrict__ out) {
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
        double f, df;
        focal_elem((double)logits[i], (double)targets[i], (double)alpha, (double)gamma, f, df);
        out[i] = gout ? (float)((double)gout[i] * df * (double)weights[i]) : (float)(f * (double)weights[i]);
    }
}

// ---- the RPN's point labels: one thread per point
struct Edge {
    float o[3], v[3][3], vv[3];
};
__device__ __forceinline__ Edge edges_of(const float* __restrict__ c) {      // c [8,3]: edges c5 - c4, c0 - c4, c7 - c4
    Edge e;
    const int far[3] = {5, 0, 7};
#pragma unroll
    for (int a = 0; a < 3; ++a) e.o[a] = c[4 * 3 + a];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int a = 0; a < 3; ++a) e.v[j][a] = c[far[j] * 3 + a] - e.o[a];
        e.vv[j] = e.v[j][0] * e.v[j][0] + e.v[j][1] * e.v[j][1] + e.v[j][2] * e.v[j][2];
    }
    return e;
}
__device__ __forceinline__ bool inside(const Edge& e, const float* p) {
    const float d[3] = {p[0] - e.o[0], p[1] - e.o[1], p[2] - e.o[2]};
    bool in = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float m = d[0] * e.v[j][0] + d[1] * e.v[j][1] + d[2] * e.v[j][2];
        in = in && (0.f < m) && (m < e.vv[j]);
    }
    return in;
}

__global__ __launch_bounds__(kThreads) void rpn_labels_kernel(const float* __restrict__ pts, const float* __restrict__ boxes,
                                                              const float* __restrict__ corners, const float* __restrict__ corners_large,
                                                              int N, float* __restrict__ cls_label, float* __restrict__ reg_label) {
    const int b = blockIdx.y;
    const int n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    const Edge e = edges_of(corners + (long)b * 24), el = edges_of(corners_large + (long)b * 24);
    const float* p = pts + ((long)b * N + n) * 3;
    const float q[3] = {p[0], p[1], p[2]};
    const bool cs = inside(e, q), big = inside(el, q);
    cls_label[(long)b * N + n] = big != cs ? -1.f : (cs ? 1.f : 0.f);
    const float* bx = boxes + (long)b * 7;
    float* r = reg_label + ((long)b * N + n) * 7;
    if (cs) {
        r[0] = bx[0] - q[0];
        r[1] = (bx[1] - bx[3] / 2.f) - q[1];
        r[2] = bx[2] - q[2];
        r[3] = bx[3]; r[4] = bx[4]; r[5] = bx[5]; r[6] = bx[6];
    } else {
#pragma unroll
        for (int i = 0; i < 7; ++i) r[i] = 0.f;
    }
}

// opt [8] int32 and cst [17] fp32 HOST arrays -> the kernel's configuration; false when the layout is not supported
bool make_cfg(int C, const int32_t* opt, const float* cst, RegCfg& k) {
    if (!opt || !cst) return false;
    k.C = C; k.P = opt[0]; k.YB = opt[1]; k.H = opt[2];
    k.xz_fine = opt[3] != 0; k.y_by_bin = opt[4] != 0; k.ry_fine = opt[5] != 0; k.anchor_per_row = opt[6] != 0;
    if (k.P < 1 || k.P > 64 || k.H < 1 || k.H > 64 || (k.y_by_bin && (k.YB < 1 || k.YB > 64))) return false;
    k.x_res = 2 * k.P; k.z_res = 3 * k.P;
    k.y_l = k.xz_fine ? 4 * k.P : 2 * k.P;
    k.y_res = k.y_l + k.YB;
    k.ry_l = k.y_by_bin ? k.y_l + 2 * k.YB : k.y_l + 1;
    k.ry_res = k.ry_l + k.H;
    k.size_l = k.ry_res + k.H;
    if (C != k.size_l + 3 || C > 128) return false;
    return true;
}
void set_consts(const float* cst, RegCfg& k) {
    k.loc_scope = cst[0]; k.loc_clamp = cst[1]; k.loc_bin = cst[2]; k.loc_half_bin = cst[3];
    k.y_scope = cst[4]; k.y_clamp = cst[5]; k.y_bin = cst[6]; k.y_half_bin = cst[7];
    k.apc = cst[8]; k.half_apc = cst[9]; k.two_pi = cst[10]; k.pi = cst[11]; k.half_pi = cst[12]; k.three_half_pi = cst[13];
    k.quarter_pi = cst[14]; k.ry_lo = cst[15]; k.ry_hi = cst[16];
}

inline unsigned reg_grid(int64_t rows) {
    int64_t b = (rows + 8 * kWaves - 1) / (8 * kWaves);          // about 8 rows per wave
    return (unsigned)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}
inline unsigned cls_grid(int64_t n) {
    int64_t b = (n + kThreads - 1) / kThreads;
    return (unsigned)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

}  // namespace

extern "C" {

int drc_train_scratch_doubles(void) { return kMaxBlocks * kSlots; }

int drc_rpn_point_labels(int B, int N, const float* pts, const float* boxes, const float* corners, const float* corners_large,
                         float* cls_label, float* reg_label, void* stream) {
    if (B < 0 || N < 0 || B > 65535) return -2;
    if (B == 0 || N == 0) return 0;
    if (!pts || !boxes || !corners || !corners_large || !cls_label || !reg_label) return -1;
    hipLaunchKernelGGL(rpn_labels_kernel, dim3((N + kThreads - 1) / kThreads, B), dim3(kThreads), 0, (hipStream_t)stream, pts, boxes, corners,
                       corners_large, N, cls_label, reg_label);
    return (int)hipGetLastError();
}

int drc_bin_reg_targets(int64_t rows, int C, const float* reg_label, const float* anchor, const int32_t* opt, const float* cst,
                        int32_t* bins, float* res, void* stream) {
    RegCfg k;
    if (rows < 0) return -2;
    if (!make_cfg(C, opt, cst, k)) return -3;
    set_consts(cst, k);
    if (rows == 0) return 0;
    if (!reg_label || !anchor || !bins || !res) return -1;
    hipLaunchKernelGGL(reg_targets_kernel, dim3((unsigned)((rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, reg_label,
                       anchor, (long)rows, k, bins, res);
    return (int)hipGetLastError();
}

int drc_bin_reg_loss_fwd(int64_t rows, int C, const float* pred_reg, const float* reg_label, const uint8_t* row_mask,
                         const uint8_t* loss_mask, const float* anchor, const int32_t* opt, const float* cst, double* sums, float* terms,
                         double* scratch, void* stream) {
    RegCfg k;
    if (rows < 0) return -2;
    if (!make_cfg(C, opt, cst, k)) return -3;
    set_consts(cst, k);
    if (!sums || !terms || !scratch) return -1;
    if (rows > 0 && (!pred_reg || !reg_label || !row_mask || !anchor)) return -1;
    unsigned blocks = 0;
    if (rows > 0) {
        blocks = reg_grid(rows);
        hipLaunchKernelGGL(reg_fwd_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, pred_reg, reg_label, row_mask, loss_mask, anchor,
                           (long)rows, k, scratch);
    }
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (const double*)scratch, (int)blocks, 0,
                       loss_mask != nullptr ? 1 : 0, k.xz_fine, k.y_by_bin, sums, terms);
    return (int)hipGetLastError();
}

int drc_bin_reg_loss_bwd(int64_t rows, int C, const float* pred_reg, const float* reg_label, const uint8_t* row_mask,
                         const uint8_t* loss_mask, const float* anchor, const int32_t* opt, const float* cst, const double* sums,
                         const float* g_loc, const float* g_angle, const float* g_size, float* grad_pred, void* stream) {
    RegCfg k;
    if (rows < 0) return -2;
    if (!make_cfg(C, opt, cst, k)) return -3;
    set_consts(cst, k);
    if (rows == 0) return 0;
    if (!pred_reg || !reg_label || !row_mask || !anchor || !sums || !grad_pred) return -1;
    hipLaunchKernelGGL(reg_bwd_kernel, dim3(reg_grid(rows)), dim3(kThreads), 0, (hipStream_t)stream, pred_reg, reg_label, row_mask, loss_mask,
                       anchor, (long)rows, k, sums, g_loc, g_angle, g_size, grad_pred);
    return (int)hipGetLastError();
}

int drc_point_cls_loss_fwd(int64_t n, int kind, const float* logits, const float* labels, const uint8_t* mask, float fg_weight, float alpha,
                           float gamma, float ignore_target, double* sums, float* terms, double* scratch, void* stream) {
    if (n < 0) return -2;
    if (kind < 1 || kind > 3) return -3;
    if (!sums || !terms || !scratch) return -1;
    if (n > 0 && (!logits || !labels)) return -1;
    const ClsCfg k = {kind, fg_weight, alpha, gamma, ignore_target};
    unsigned blocks = 0;
    if (n > 0) {
        blocks = cls_grid(n);
        hipLaunchKernelGGL(cls_fwd_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, logits, labels, mask, (long)n, k, scratch);
    }
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (const double*)scratch, (int)blocks, kind, 0, 0, 0, sums,
                       terms);
    return (int)hipGetLastError();
}

int drc_point_cls_loss_bwd(int64_t n, int kind, const float* logits, const float* labels, const uint8_t* mask, float fg_weight, float alpha,
                           float gamma, float ignore_target, const double* sums, const float* grad_out, float* grad_logits, void* stream) {
    if (n < 0) return -2;
    if (kind < 1 || kind > 3) return -3;
    if (n == 0) return 0;
    if (!logits || !labels || !sums || !grad_out || !grad_logits) return -1;
    const ClsCfg k = {kind, fg_weight, alpha, gamma, ignore_target};
    hipLaunchKernelGGL(cls_bwd_kernel, dim3(cls_grid(n)), dim3(kThreads), 0, (hipStream_t)stream, logits, labels, mask, (long)n, k, sums,
                       grad_out, grad_logits);
    return (int)hipGetLastError();
}

int drc_focal_elementwise(int64_t n, const float* logits, const float* targets, const float* weights, float alpha, float gamma,
                          const float* grad_out, float* out, void* stream) {
    if (n < 0) return -2;
    if (n == 0) return 0;
    if (!logits || !targets || !weights || !out) return -1;
    hipLaunchKernelGGL(focal_elem_kernel, dim3(cls_grid(n)), dim3(kThreads), 0, (hipStream_t)stream, logits, targets, weights, (long)n, alpha,
                       gamma, grad_out, out);
    return (int)hipGetLastError();
}

}  // extern "C"

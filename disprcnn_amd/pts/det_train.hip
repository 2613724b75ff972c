// det_train.hip -- training targets, balanced sampling and losses of the stereo 2D stage (gfx950).
//
//   reference: modeling/rpn/stereo_rpn/loss.py, modeling/roi_heads/box_head/loss.py, modeling/matcher.py,
//              modeling/balanced_positive_negative_sampler.py, modeling/box_coder.py (encode_*), utils/stereo_utils.py
//              (expand_left_right_box), structures/boxlist_ops.py (boxlist_iou), layers/smooth_l1_loss.py, modeling/rpn/utils.py,
//              modeling/roi_heads/mask_head/loss.py, structures/segmentation_mask.py (BinaryMaskList.crop / .resize; mask_resize.h).
//
// Everything that decides a label, a match or a tie is fp32 in the reference's operation order (the library builds with
// -ffp-contract=off), so a candidate lands where the reference puts it.  Loss values are evaluated and summed in fp64: per-block partials,
// added in block order by a finishing launch.  No float atomics, no host read: two runs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_pts.h"
#include "mask_resize.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSelThreads = 1024;
constexpr int kMaxImages = DRC_DET2D_MAX_IMAGES;
constexpr int kMaxGT = DRC_DET2D_MAX_GT;
constexpr int kMaxLevels = DRC_DET2D_MAX_LEVELS;

struct Spans {                       // CSR offsets of the images' candidates and ground truths, by value: no upload
    int32_t cand[kMaxImages + 1];
    int32_t gt[kMaxImages + 1];
};

__device__ __forceinline__ float iou_legacy(const float* t, float area1, float x1, float y1, float x2, float y2, float area2) {
    float w = (fminf(t[2], x2) - fmaxf(t[0], x1)) + 1.f;
    float h = (fminf(t[3], y2) - fmaxf(t[1], y1)) + 1.f;
    w = w < 0.f ? 0.f : w;
    h = h < 0.f ? 0.f : h;
    const float inter = w * h;
    return inter / ((area1 + area2) - inter);
}
// the order of non-negative floats is the order of their bit patterns
__device__ __forceinline__ unsigned iou_key(float v) { return v > 0.f ? __float_as_uint(v) : 0u; }

// union boxes (expand_left_right_box) and areas of image n's ground truths -> LDS [ng][5]
__device__ __forceinline__ void stage_gt(float* s_gt, const float* __restrict__ gl, const float* __restrict__ gr, int g0, int ng) {
    for (int g = threadIdx.x; g < ng; g += blockDim.x) {
        const float* l = gl + (int64_t)(g0 + g) * 4;
        const float* r = gr + (int64_t)(g0 + g) * 4;
        const float x1 = fminf(l[0], r[0]), y1 = fminf(l[1], r[1]), x2 = fmaxf(l[2], r[2]), y2 = fmaxf(l[3], r[3]);
        s_gt[g * 5 + 0] = x1; s_gt[g * 5 + 1] = y1; s_gt[g * 5 + 2] = x2; s_gt[g * 5 + 3] = y2;
        s_gt[g * 5 + 4] = (x2 - x1 + 1.f) * (y2 - y1 + 1.f);
    }
}
// a candidate's box for the IoU: itself (4 coordinates) or the union of its two views (6: x1 y1 x2 y2 x1' x2')
__device__ __forceinline__ void cand_box(const float* __restrict__ c, int cs, float* b) {
    if (cs == 6) { b[0] = fminf(c[0], c[4]); b[1] = c[1]; b[2] = fmaxf(c[2], c[5]); b[3] = c[3]; }
    else { b[0] = c[0]; b[1] = c[1]; b[2] = c[2]; b[3] = c[3]; }
}

// ---- 1. matching ------------------------------------------------------------------------------------------------------------
// per-ground-truth maximum over all candidates of the image (only with low-quality matches)
__global__ __launch_bounds__(kThreads) void gt_max_kernel(Spans sp, int cs, const float* __restrict__ cand, const float* __restrict__ gl,
                                                          const float* __restrict__ gr, unsigned* __restrict__ gt_max) {
    __shared__ float s_gt[kMaxGT * 5];
    __shared__ unsigned s_max[kMaxGT];
    const int n = blockIdx.y;
    const int c0 = sp.cand[n], c1 = sp.cand[n + 1], g0 = sp.gt[n];
    int ng = sp.gt[n + 1] - g0;
    if (ng > kMaxGT) ng = kMaxGT;
    if ((int64_t)blockIdx.x * kThreads >= c1 - c0) return;           // block-uniform
    stage_gt(s_gt, gl, gr, g0, ng);
    for (int g = threadIdx.x; g < ng; g += kThreads) s_max[g] = 0u;
    __syncthreads();
    const int i = c0 + blockIdx.x * kThreads + threadIdx.x;
    const bool valid = i < c1;
    float b[4] = {0.f, 0.f, 0.f, 0.f};
    if (valid) cand_box(cand + (int64_t)i * cs, cs, b);
    const float area2 = (b[2] - b[0] + 1.f) * (b[3] - b[1] + 1.f);
    for (int g = 0; g < ng; ++g) {
        unsigned v = valid ? iou_key(iou_legacy(s_gt + g * 5, s_gt[g * 5 + 4], b[0], b[1], b[2], b[3], area2)) : 0u;
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned o = (unsigned)__shfl_xor((int)v, off);
            v = o > v ? o : v;
        }
        if ((threadIdx.x & 63) == 0 && v) atomicMax(&s_max[g], v);
    }
    __syncthreads();
    for (int g = threadIdx.x; g < ng; g += kThreads)
        if (s_max[g]) atomicMax(&gt_max[g0 + g], s_max[g]);
}

__global__ __launch_bounds__(kThreads) void match_kernel(Spans sp, int cs, const float* __restrict__ cand, const float* __restrict__ gl,
                                                         const float* __restrict__ gr, const int64_t* __restrict__ gt_labels,
                                                         const uint8_t* __restrict__ visibility, float high, float low,
                                                         const unsigned* __restrict__ gt_max, float wx, float wy, float ww, float wh,
                                                         int64_t* __restrict__ matched, float* __restrict__ labels_f,
                                                         int64_t* __restrict__ labels_l, float* __restrict__ reg) {
    __shared__ float s_gt[kMaxGT * 5];
    const int n = blockIdx.y;
    const int c0 = sp.cand[n], c1 = sp.cand[n + 1], g0 = sp.gt[n];
    int ng = sp.gt[n + 1] - g0;
    if (ng > kMaxGT) ng = kMaxGT;
    if ((int64_t)blockIdx.x * kThreads >= c1 - c0) return;           // block-uniform
    stage_gt(s_gt, gl, gr, g0, ng);
    __syncthreads();
    const int i = c0 + blockIdx.x * kThreads + threadIdx.x;
    if (i >= c1 || ng <= 0) return;
    const float* c = cand + (int64_t)i * cs;
    float p[6];
    for (int k = 0; k < cs; ++k) p[k] = c[k];
    float b[4];
    cand_box(p, cs, b);
    const float area2 = (b[2] - b[0] + 1.f) * (b[3] - b[1] + 1.f);
    float best = -1.f;
    int arg = 0;
    bool rescued = false;
    for (int g = 0; g < ng; ++g) {
        const float iou = iou_legacy(s_gt + g * 5, s_gt[g * 5 + 4], b[0], b[1], b[2], b[3], area2);
        if (g == 0 || iou > best) { best = iou; arg = g; }
        if (gt_max && iou_key(iou) == gt_max[g0 + g]) rescued = true;     // set_low_quality_matches_: ties included, a maximum of 0 too
    }
    int64_t m = arg;
    if (best < low) m = -1;
    else if (best < high) m = -2;
    if (rescued) m = arg;
    matched[i] = m;
    const int64_t tg = g0 + (m < 0 ? 0 : m);                               // target[matched_idxs.clamp(min=0)]
    int64_t label = gt_labels ? gt_labels[tg] : (m >= 0 ? 1 : 0);
    if (m == -1) label = 0;
    if (m == -2) label = -1;
    if (visibility && !visibility[i]) label = -1;
    if (labels_f) labels_f[i] = (float)label;
    if (labels_l) labels_l[i] = label;
    // original_lr_bbox of the target: (left x1, union y1, left x2, union y2, right x1, right x2)
    const float* l = gl + tg * 4;
    const float* r = gr + tg * 4;
    const float t[6] = {l[0], fminf(l[1], r[1]), l[2], fmaxf(l[3], r[3]), r[0], r[2]};
    const float ew = p[2] - p[0] + 1.f, eh = p[3] - p[1] + 1.f;
    const float ex = p[0] + 0.5f * ew, ey = p[1] + 0.5f * eh;
    float ewp = ew, exp_ = ex;                                             // ..._fromboxes4: the right view is coded against the same box
    if (cs == 6) { ewp = p[5] - p[4] + 1.f; exp_ = p[4] + 0.5f * ewp; }
    const float gw = t[2] - t[0] + 1.f, gh = t[3] - t[1] + 1.f, gwp = t[5] - t[4] + 1.f;
    const float gx = t[0] + 0.5f * gw, gy = t[1] + 0.5f * gh, gxp = t[4] + 0.5f * gwp;
    float* o = reg + (int64_t)i * 6;
    o[0] = wx * (gx - ex) / ew;
    o[1] = wy * (gy - ey) / eh;
    o[2] = ww * logf(gw / ew);
    o[3] = wh * logf(gh / eh);
    o[4] = wx * (gxp - exp_) / ewp;
    o[5] = ww * logf(gwp / ewp);
}

// ---- 2. balanced sampling ---------------------------------------------------------------------------------------------------
// class of a candidate: 1 positive, 0 negative, -1 ignored
__device__ __forceinline__ int label_class(const void* labels, int kind, int64_t i) {
    if (kind == 0) { const float v = ((const float*)labels)[i]; return v >= 1.f ? 1 : (v == 0.f ? 0 : -1); }
    const int64_t v = ((const int64_t*)labels)[i];
    return v >= 1 ? 1 : (v == 0 ? 0 : -1);
}
__device__ __forceinline__ unsigned draw_key(float d) { return __float_as_uint(d + 0.f); }   // -0 -> +0

// One workgroup per (class, image).  The k members with the smallest (draw, index) keys: a radix select on the draw's bit pattern, eight
// bits a pass from the top, finds the k-th draw T and how many of the members that draw exactly T are still wanted; an ordered scan then
// takes everything below T and the first of the ties in index order.
__global__ __launch_bounds__(kSelThreads) void balanced_sample_kernel(Spans sp, const void* __restrict__ labels, int kind,
                                                                      const float* __restrict__ draws, int batch, int cap_pos,
                                                                      uint8_t* __restrict__ pos_mask, uint8_t* __restrict__ neg_mask,
                                                                      int32_t* __restrict__ counts) {
    __shared__ unsigned s_hist[256];
    __shared__ unsigned s_cnt[2];
    __shared__ unsigned s_prefix, s_remain;
    __shared__ unsigned s_wave[kSelThreads / 64];
    const int cls = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const int want = cls == 0 ? 1 : 0;
    const int c0 = sp.cand[n], c1 = sp.cand[n + 1];
    if (tid < 2) s_cnt[tid] = 0u;
    __syncthreads();
    unsigned lp = 0, ln = 0;
    for (int i = c0 + tid; i < c1; i += kSelThreads) {
        const int c = label_class(labels, kind, i);
        lp += c == 1;
        ln += c == 0;
    }
    for (int off = 32; off > 0; off >>= 1) {
        lp += (unsigned)__shfl_xor((int)lp, off);
        ln += (unsigned)__shfl_xor((int)ln, off);
    }
    if ((tid & 63) == 0) { atomicAdd(&s_cnt[0], lp); atomicAdd(&s_cnt[1], ln); }
    __syncthreads();
    const unsigned npos = s_cnt[0], nneg = s_cnt[1];
    const unsigned num_pos = npos < (unsigned)cap_pos ? npos : (unsigned)cap_pos;
    const unsigned room = (unsigned)batch > num_pos ? (unsigned)batch - num_pos : 0u;
    const unsigned num_neg = nneg < room ? nneg : room;
    const unsigned nmem = cls == 0 ? npos : nneg, k = cls == 0 ? num_pos : num_neg;
    uint8_t* __restrict__ mask = cls == 0 ? pos_mask : neg_mask;
    if (tid == 0) counts[n * 2 + cls] = (int32_t)k;
    if (k == 0u || k >= nmem) {                                          // block-uniform: nobody, or every member
        for (int i = c0 + tid; i < c1; i += kSelThreads) mask[i] = (k > 0u && label_class(labels, kind, i) == want) ? 1 : 0;
        return;
    }
    unsigned prefix = 0u, remain = k;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned hmask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
        if (tid < 256) s_hist[tid] = 0u;
        __syncthreads();
        for (int i = c0 + tid; i < c1; i += kSelThreads) {
            if (label_class(labels, kind, i) != want) continue;
            const unsigned key = draw_key(draws[i]);
            if ((key & hmask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned cum = 0u, bin = 255u, left = remain;
            for (unsigned bb = 0; bb < 256u; ++bb) {
                const unsigned h = s_hist[bb];
                if (cum + h >= remain) { bin = bb; left = remain - cum; break; }
                cum += h;
            }
            s_prefix = prefix | (bin << shift);
            s_remain = left;
        }
        __syncthreads();
        prefix = s_prefix;
        remain = s_remain;
        __syncthreads();
    }
    const unsigned T = prefix;
    unsigned base = 0u;
    const int lane = tid & 63, wave = tid >> 6;
    for (int start = c0; start < c1; start += kSelThreads) {             // block-uniform trip count
        const int i = start + tid;
        const bool member = i < c1 && label_class(labels, kind, i) == want;
        const unsigned key = member ? draw_key(draws[i]) : 0u;
        const bool tie = member && key == T;
        const unsigned long long bal = __ballot(tie);
        const unsigned rank = (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = (unsigned)__popcll(bal);
        __syncthreads();
        unsigned wbase = 0u, total = 0u;
        for (int w = 0; w < kSelThreads / 64; ++w) {
            const unsigned c = s_wave[w];
            wbase += w < wave ? c : 0u;
            total += c;
        }
        if (i < c1) mask[i] = (member && (key < T || (tie && base + wbase + rank < remain))) ? 1 : 0;
        base += total;
        __syncthreads();
    }
}

// the sampled candidates of each image in ascending index order (nonzero(pos | neg)), image-local, -1 past the count
__global__ __launch_bounds__(kSelThreads) void compact_kernel(Spans sp, const uint8_t* __restrict__ pos_mask,
                                                              const uint8_t* __restrict__ neg_mask, int batch, int64_t* __restrict__ out) {
    __shared__ unsigned s_wave[kSelThreads / 64];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = sp.cand[n], c1 = sp.cand[n + 1];
    int64_t* __restrict__ o = out + (int64_t)n * batch;
    unsigned base = 0u;
    for (int start = c0; start < c1; start += kSelThreads) {
        const int i = start + tid;
        const bool sel = i < c1 && (pos_mask[i] | neg_mask[i]);
        const unsigned long long bal = __ballot(sel);
        const unsigned rank = (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = (unsigned)__popcll(bal);
        __syncthreads();
        unsigned wbase = 0u, total = 0u;
        for (int w = 0; w < kSelThreads / 64; ++w) {
            const unsigned c = s_wave[w];
            wbase += w < wave ? c : 0u;
            total += c;
        }
        const unsigned at = base + wbase + rank;
        if (sel && at < (unsigned)batch) o[at] = i - c0;
        base += total;
        __syncthreads();
    }
    for (unsigned r = base + tid; r < (unsigned)batch; r += kSelThreads) o[r] = -1;
}

// ---- reductions -------------------------------------------------------------------------------------------------------------
// the block's sums of K values -> part[K], waves added in wave order
template <int K>
__device__ __forceinline__ void block_partials(double (&v)[K], double* __restrict__ part) {
    __shared__ double s[kThreads / 64][K];
    for (int k = 0; k < K; ++k)
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < K; ++k) s[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < K; ++k) {
            double t = 0.0;
            for (int w = 0; w < kThreads / 64; ++w) t += s[w][k];
            part[k] = t;
        }
}

// one workgroup: the partials in block order; terms[k] = sum_k / denom (0 when denom is 0), terms[K] = denom.  denom is `denom` or, with
// `counts`, the sum of its n_counts entries.
__global__ __launch_bounds__(kThreads) void finish_kernel(const double* __restrict__ part, int64_t blocks, int K,
                                                          const int32_t* __restrict__ counts, int n_counts, double denom,
                                                          double count_scale, float* __restrict__ terms) {
    __shared__ double s[kThreads];
    for (int k = 0; k < K; ++k) {
        double t = 0.0;
        for (int64_t b = threadIdx.x; b < blocks; b += kThreads) t += part[b * K + k];
        s[threadIdx.x] = t;
        __syncthreads();
        if (threadIdx.x == 0) {
            double d = denom;
            if (counts) {
                int64_t c = 0;
                for (int i = 0; i < n_counts; ++i) c += counts[i];
                d = (double)c * count_scale;
            }
            double sum = 0.0;
            for (int i = 0; i < kThreads; ++i) sum += s[i];
            terms[k] = d > 0.0 ? (float)(sum / d) : 0.f;
            terms[K] = (float)d;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ double smooth_l1(double d, double beta, double* grad) {
    const double a = fabs(d);
    if (a < beta) { *grad = d / beta; return 0.5 * a * a / beta; }
    *grad = d > 0.0 ? 1.0 : -1.0;
    return a - 0.5 * beta;
}

// ---- 3. Stereo RPN loss -----------------------------------------------------------------------------------------------------
struct SrpnLevels {
    const float* logits[kMaxLevels];
    const float* bbox[kMaxLevels];
    float* glogits[kMaxLevels];
    float* gbbox[kMaxLevels];
    int32_t H[kMaxLevels], W[kMaxLevels], off[kMaxLevels];
};

// the head's pair softmax: probability of raw channel ch (paired with ch + A, or ch - A) and of its partner
__device__ __forceinline__ void pair_prob(const float* __restrict__ z, int64_t HW, int A, int ch, double* q, double* r) {
    const int other = ch < A ? ch + A : ch - A;
    const double d = (double)z[(int64_t)other * HW] - (double)z[(int64_t)ch * HW];
    *q = 1.0 / (1.0 + exp(d));
    *r = 1.0 / (1.0 + exp(-d));
}
// d loss / d probability map channel ch, times the sampled count: channel ch is entry ch & 1 of anchor ch >> 1's objectness vector
__device__ __forceinline__ double prob_grad(const float* __restrict__ z, int64_t HW, int A, int ch, int64_t loc_anchor0,
                                            const uint8_t* __restrict__ pos_mask, const uint8_t* __restrict__ neg_mask) {
    const int a = ch >> 1, j = ch & 1;
    const int pos = pos_mask[loc_anchor0 + a], neg = neg_mask[loc_anchor0 + a];
    if (!(pos | neg)) return 0.0;
    double p0, p1, unused;
    pair_prob(z, HW, A, 2 * a, &p0, &unused);
    pair_prob(z, HW, A, 2 * a + 1, &p1, &unused);
    const double sj = 1.0 / (1.0 + exp(j ? p0 - p1 : p1 - p0));           // softmax of (p0, p1), entry j
    return sj - ((pos ? 1 : 0) == j ? 1.0 : 0.0);
}

// A thread owns anchor a of one location: its loss terms, the six box-code gradients, and the raw pair (a, a + A) of the location.
__global__ __launch_bounds__(kThreads) void srpn_loss_kernel(SrpnLevels lv, int N, int A, int64_t total, const uint8_t* __restrict__ pos_mask,
                                                             const uint8_t* __restrict__ neg_mask, const float* __restrict__ reg_targets,
                                                             const int32_t* __restrict__ counts, double beta, double* __restrict__ part) {
    __shared__ double s_inv;
    const int l = blockIdx.y;
    const int H = lv.H[l], W = lv.W[l];
    const int64_t HW = (int64_t)H * W, per = (int64_t)N * A * HW;
    if (threadIdx.x == 0) {
        int64_t c = 0;
        for (int i = 0; i < 2 * N; ++i) c += counts[i];
        s_inv = c > 0 ? 1.0 / (double)c : 0.0;
    }
    __syncthreads();
    const double inv = s_inv;
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double v[2] = {0.0, 0.0};
    if (t < per) {
        const int64_t pix = t % HW;
        const int a = (int)((t / HW) % A);
        const int n = (int)(t / (HW * A));
        const float* __restrict__ z = lv.logits[l] + (int64_t)n * 2 * A * HW + pix;
        const int64_t anchor0 = (int64_t)n * total + lv.off[l] + pix * A;
        const int64_t i = anchor0 + a;
        const int pos = pos_mask[i], neg = neg_mask[i];
        if (pos | neg) {
            double p0, p1, unused;
            pair_prob(z, HW, A, 2 * a, &p0, &unused);
            pair_prob(z, HW, A, 2 * a + 1, &p1, &unused);
            const double m = p0 > p1 ? p0 : p1;
            v[0] = m + log(exp(p0 - m) + exp(p1 - m)) - (pos ? p1 : p0);
        }
        const float* __restrict__ bb = lv.bbox[l] + ((int64_t)n * 6 * A + (int64_t)a * 6) * HW + pix;
        float* __restrict__ gb = lv.gbbox[l] + ((int64_t)n * 6 * A + (int64_t)a * 6) * HW + pix;
        for (int k = 0; k < 6; ++k) {
            double g = 0.0;
            if (pos) v[1] += smooth_l1((double)bb[k * HW] - (double)reg_targets[i * 6 + k], beta, &g);
            gb[k * HW] = (float)(g * inv);
        }
        double q, r;
        pair_prob(z, HW, A, a, &q, &r);
        const double dz = q * r * (prob_grad(z, HW, A, a, anchor0, pos_mask, neg_mask) - prob_grad(z, HW, A, a + A, anchor0, pos_mask, neg_mask)) * inv;
        float* __restrict__ gz = lv.glogits[l] + (int64_t)n * 2 * A * HW + pix;
        gz[(int64_t)a * HW] = (float)dz;
        gz[(int64_t)(a + A) * HW] = (float)(-dz);
    }
    block_partials<2>(v, part + ((int64_t)l * gridDim.x + blockIdx.x) * 2);
}

// ---- 4. box-head loss -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void fastrcnn_loss_kernel(int R, int C, const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                                 const float* __restrict__ box, const float* __restrict__ reg_targets,
                                                                 float* __restrict__ glogits, float* __restrict__ gbox,
                                                                 double* __restrict__ part) {
    const int r = blockIdx.x * kThreads + threadIdx.x;
    double v[2] = {0.0, 0.0};
    if (r < R) {
        const double inv = 1.0 / (double)R;
        const float* __restrict__ x = logits + (int64_t)r * C;
        const int64_t lab = labels[r];
        const bool ok = lab >= 0 && lab < C;                             // rows with a label outside [0, C) carry nothing
        double m = (double)x[0];
        for (int c = 1; c < C; ++c) m = (double)x[c] > m ? (double)x[c] : m;
        double se = 0.0;
        for (int c = 0; c < C; ++c) se += exp((double)x[c] - m);
        const double lse = m + log(se);
        if (ok) v[0] = lse - (double)x[lab];
        for (int c = 0; c < C; ++c)
            glogits[(int64_t)r * C + c] = ok ? (float)((exp((double)x[c] - lse) - (c == lab ? 1.0 : 0.0)) * inv) : 0.f;
        const float* __restrict__ b = box + (int64_t)r * 6 * C;
        float* __restrict__ gb = gbox + (int64_t)r * 6 * C;
        for (int j = 0; j < 6 * C; ++j) {
            double g = 0.0;
            if (ok && lab > 0 && j >= 6 * lab && j < 6 * lab + 6)
                v[1] += smooth_l1((double)b[j] - (double)reg_targets[(int64_t)r * 6 + (j - 6 * lab)], 1.0, &g);
            gb[j] = (float)(g * inv);
        }
    }
    block_partials<2>(v, part + (int64_t)blockIdx.x * 2);
}

// ---- 5. mask targets and loss -----------------------------------------------------------------------------------------------
// The ROI's instance and class: the target at the matched row clamped at 0 (so a row between the thresholds reads row 0, as the reference's
// target[matched_idxs.clamp(min=0)] does), nothing where the match fell below the low threshold.  -1: not a positive ROI.
__device__ __forceinline__ int64_t mask_instance(const Spans& sp, int N, int p, const int64_t* __restrict__ matched,
                                                 const int64_t* __restrict__ inst_labels, int C, int* cls) {
    int n = 0;
    while (n + 1 < N && p >= sp.cand[n + 1]) ++n;
    const int64_t m = matched[p];
    const int64_t inst = sp.gt[n] + (m < 0 ? 0 : m);
    if (m == -1 || inst >= sp.gt[n + 1]) return -1;
    const int64_t c = inst_labels[inst];
    if (c <= 0 || c >= C) return -1;
    *cls = (int)c;
    return inst;
}

__global__ __launch_bounds__(kThreads) void mask_count_kernel(Spans sp, int N, int P, int C, const int64_t* __restrict__ matched,
                                                              const int64_t* __restrict__ inst_labels, int32_t* __restrict__ count) {
    __shared__ unsigned s_cnt;
    if (threadIdx.x == 0) s_cnt = 0u;
    __syncthreads();
    unsigned c = 0;
    int cls;
    for (int p = threadIdx.x; p < P; p += kThreads) c += mask_instance(sp, N, p, matched, inst_labels, C, &cls) >= 0;
    if (c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) count[0] = (int32_t)s_cnt;
}

// One workgroup per ROI: crop bounds, the M x M target, the loss of the ROI's class plane and the gradient of all C planes.
__global__ __launch_bounds__(kThreads) void mask_loss_kernel(Spans sp, int N, int C, int M, const float* __restrict__ boxes,
                                                             const int64_t* __restrict__ matched, const int64_t* __restrict__ inst_labels,
                                                             const float* __restrict__ logits, const uint8_t* __restrict__ masks,
                                                             const int64_t* __restrict__ table, const int32_t* __restrict__ count,
                                                             uint8_t* __restrict__ targets, float* __restrict__ grad,
                                                             double* __restrict__ part) {
    const int p = blockIdx.x, MM = M * M;
    int cls = 0;
    const int64_t inst = mask_instance(sp, N, p, matched, inst_labels, C, &cls);
    double v[1] = {0.0};
    float* __restrict__ g = grad + (int64_t)p * C * MM;
    uint8_t* __restrict__ tg = targets + (int64_t)p * MM;
    if (inst < 0) {                                                      // block-uniform
        for (int e = threadIdx.x; e < C * MM; e += kThreads) g[e] = 0.f;
        for (int e = threadIdx.x; e < MM; e += kThreads) tg[e] = 0;
    } else {
        const int H = (int)table[inst * 3 + 1], W = (int)table[inst * 3 + 2];
        const uint8_t* __restrict__ mask = masks + table[inst * 3 + 0];
        const drc_mask::Crop crop = drc_mask::crop_bounds(boxes + (int64_t)p * 4, W, H);
        const double inv = 1.0 / ((double)count[0] * (double)MM);
        const float* __restrict__ x = logits + ((int64_t)p * C + cls) * MM;
        for (int e = threadIdx.x; e < C * MM; e += kThreads) {
            const int c = e / MM, pix = e - c * MM;
            float gv = 0.f;
            if (c == cls) {
                const int oy = pix / M, ox = pix - oy * M;
                const uint8_t t = (uint8_t)drc_mask::resize_pixel(mask, W, crop, M, oy, ox);      // truncation: 1 only at 1.0
                tg[pix] = t;
                const double xv = (double)x[pix], a = fabs(xv);
                v[0] += (xv > 0.0 ? xv : 0.0) - xv * (double)t + log1p(exp(-a));
                const double s = xv >= 0.0 ? 1.0 / (1.0 + exp(-xv)) : exp(xv) / (1.0 + exp(xv));
                gv = (float)((s - (double)t) * inv);
            }
            g[e] = gv;
        }
    }
    block_partials<1>(v, part + p);
}

bool fill_spans(Spans& sp, int N, const int32_t* cand_off, const int32_t* gt_off) {
    if (N < 1 || N > kMaxImages || !cand_off || cand_off[0] != 0) return false;
    for (int n = 0; n <= N; ++n) {
        sp.cand[n] = cand_off[n];
        sp.gt[n] = gt_off ? gt_off[n] : 0;
        if (n && (sp.cand[n] < sp.cand[n - 1] || sp.gt[n] < sp.gt[n - 1])) return false;
    }
    if (gt_off && gt_off[0] != 0) return false;
    for (int n = N + 1; n <= kMaxImages; ++n) { sp.cand[n] = sp.cand[N]; sp.gt[n] = sp.gt[N]; }
    return true;
}
int max_span(const Spans& sp, int N) {
    int m = 0;
    for (int n = 0; n < N; ++n) m = sp.cand[n + 1] - sp.cand[n] > m ? sp.cand[n + 1] - sp.cand[n] : m;
    return m;
}

}  // namespace

extern "C" int drc_det2d_max_gt(void) { return kMaxGT; }
extern "C" int drc_det2d_max_images(void) { return kMaxImages; }

extern "C" int drc_det2d_match_fwd(int N, const int32_t* cand_off, const int32_t* gt_off, int cs, const float* cand, const float* gt_left,
                                   const float* gt_right, const int64_t* gt_labels, const uint8_t* visibility, float high, float low,
                                   int allow_low_quality, const float* weights4, uint32_t* gt_max, int64_t* matched, float* labels_f32,
                                   int64_t* labels_i64, float* reg_targets, void* stream) {
    Spans sp;
    if ((cs != 4 && cs != 6) || !weights4 || !fill_spans(sp, N, cand_off, gt_off)) return -2;
    for (int n = 0; n < N; ++n) {
        const int ng = sp.gt[n + 1] - sp.gt[n];
        if (ng < 1 || ng > kMaxGT || sp.cand[n + 1] == sp.cand[n]) return -2;
    }
    if (!cand || !gt_left || !gt_right || !matched || !reg_targets || (!labels_f32 && !labels_i64) || (allow_low_quality && !gt_max)) return -1;
    if ((int64_t)sp.cand[N] * 6 > INT32_MAX) return -2;
    const dim3 grid((unsigned)((max_span(sp, N) + kThreads - 1) / kThreads), (unsigned)N);
    if (allow_low_quality) {
        hipError_t e = hipMemsetAsync(gt_max, 0, sizeof(uint32_t) * (size_t)sp.gt[N], (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(gt_max_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, sp, cs, cand, gt_left, gt_right, gt_max);
    }
    hipLaunchKernelGGL(match_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, sp, cs, cand, gt_left, gt_right, gt_labels, visibility, high,
                       low, allow_low_quality ? (const unsigned*)gt_max : nullptr, weights4[0], weights4[1], weights4[2], weights4[3], matched,
                       labels_f32, labels_i64, reg_targets);
    return (int)hipGetLastError();
}

extern "C" int drc_det2d_sample_fwd(int N, const int32_t* cand_off, const void* labels, int label_kind, const float* draws, int batch,
                                    int cap_pos, uint8_t* pos_mask, uint8_t* neg_mask, int32_t* counts, int64_t* sampled_idx, void* stream) {
    Spans sp;
    if (batch < 0 || cap_pos < 0 || cap_pos > batch || (label_kind != 0 && label_kind != 1) || !fill_spans(sp, N, cand_off, nullptr)) return -2;
    if (!counts || (sp.cand[N] > 0 && (!labels || !draws || !pos_mask || !neg_mask))) return -1;
    hipLaunchKernelGGL(balanced_sample_kernel, dim3(2, (unsigned)N), dim3(kSelThreads), 0, (hipStream_t)stream, sp, labels, label_kind, draws,
                       batch, cap_pos, pos_mask, neg_mask, counts);
    if (sampled_idx && batch > 0)
        hipLaunchKernelGGL(compact_kernel, dim3((unsigned)N), dim3(kSelThreads), 0, (hipStream_t)stream, sp, pos_mask, neg_mask, batch, sampled_idx);
    return (int)hipGetLastError();
}

extern "C" int64_t drc_det2d_srpn_loss_partials(int N, int A, int n_levels, const int64_t* levels) {
    if (N < 1 || A < 1 || n_levels < 1 || n_levels > kMaxLevels || !levels) return -1;
    int64_t most = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int64_t per = (int64_t)N * A * levels[l * 7 + 4] * levels[l * 7 + 5];
        most = per > most ? per : most;
    }
    return ((most + kThreads - 1) / kThreads) * n_levels * 2;
}

extern "C" int drc_det2d_srpn_loss_fwd(int N, int A, int n_levels, const int64_t* levels, int64_t total, const uint8_t* pos_mask,
                                       const uint8_t* neg_mask, const float* reg_targets, const int32_t* counts, double beta, double* partials,
                                       float* terms, void* stream) {
    if (N < 1 || N > kMaxImages || A < 1 || n_levels < 1 || n_levels > kMaxLevels || !levels || total < 1 || !(beta > 0.0)) return -2;
    if (!pos_mask || !neg_mask || !reg_targets || !counts || !partials || !terms) return -1;
    SrpnLevels lv = {};
    int64_t most = 0, covered = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int64_t* r = levels + l * 7;
        lv.logits[l] = (const float*)(uintptr_t)r[0];
        lv.bbox[l] = (const float*)(uintptr_t)r[1];
        lv.glogits[l] = (float*)(uintptr_t)r[2];
        lv.gbbox[l] = (float*)(uintptr_t)r[3];
        if (!r[0] || !r[1] || !r[2] || !r[3] || r[4] < 1 || r[5] < 1 || r[6] != covered) return -2;    // levels tile [0, total) in order
        const int64_t per = (int64_t)N * A * r[4] * r[5];
        if (per * 6 > INT32_MAX) return -2;
        lv.H[l] = (int32_t)r[4]; lv.W[l] = (int32_t)r[5]; lv.off[l] = (int32_t)r[6];
        covered += r[4] * r[5] * A;
        most = per > most ? per : most;
    }
    if (covered != total || (int64_t)N * total * 6 > INT32_MAX) return -2;
    const unsigned gx = (unsigned)((most + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(srpn_loss_kernel, dim3(gx, (unsigned)n_levels), dim3(kThreads), 0, (hipStream_t)stream, lv, N, A, total, pos_mask,
                       neg_mask, reg_targets, counts, beta, partials);
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (const double*)partials, (int64_t)gx * n_levels, 2,
                       counts, 2 * N, 0.0, 1.0, terms);
    return (int)hipGetLastError();
}

extern "C" int drc_det2d_fastrcnn_loss_fwd(int R, int C, const float* class_logits, const int64_t* labels, const float* box_regression,
                                           const float* reg_targets, float* grad_logits, float* grad_box, double* partials, float* terms,
                                           void* stream) {
    if (R < 1 || C < 1 || (int64_t)R * 6 * C > INT32_MAX) return -2;
    if (!class_logits || !labels || !box_regression || !reg_targets || !grad_logits || !grad_box || !partials || !terms) return -1;
    const unsigned gx = (unsigned)((R + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(fastrcnn_loss_kernel, dim3(gx), dim3(kThreads), 0, (hipStream_t)stream, R, C, class_logits, labels, box_regression,
                       reg_targets, grad_logits, grad_box, partials);
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (const double*)partials, (int64_t)gx, 2,
                       (const int32_t*)nullptr, 0, (double)R, 1.0, terms);
    return (int)hipGetLastError();
}

extern "C" int drc_det2d_mask_loss_fwd(int N, const int32_t* roi_off, const int32_t* inst_off, int C, int M, const float* boxes,
                                       const int64_t* matched, const int64_t* inst_labels, const float* mask_logits, const uint8_t* masks,
                                       const int64_t* table, int32_t* count, uint8_t* targets, float* grad_logits, double* partials,
                                       float* terms, void* stream) {
    Spans sp;
    if (C < 1 || M < 1 || M > 1024 || !fill_spans(sp, N, roi_off, inst_off)) return -2;
    const int P = sp.cand[N];
    if (!count || !terms) return -1;
    if ((int64_t)P * C * M * M > INT32_MAX) return -2;
    if (P > 0 && (!boxes || !matched || !inst_labels || !mask_logits || !masks || !table || !targets || !grad_logits || !partials)) return -1;
    hipLaunchKernelGGL(mask_count_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, sp, N, P, C, matched, inst_labels, count);
    if (P > 0)
        hipLaunchKernelGGL(mask_loss_kernel, dim3((unsigned)P), dim3(kThreads), 0, (hipStream_t)stream, sp, N, C, M, boxes, matched, inst_labels,
                           mask_logits, masks, table, (const int32_t*)count, targets, grad_logits, partials);
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (const double*)partials, (int64_t)P, 1,
                       (const int32_t*)count, 1, 0.0, (double)M * M, terms);
    return (int)hipGetLastError();
}

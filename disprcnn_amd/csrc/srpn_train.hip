// srpn_train.hip -- the sparse pieces of the Stereo RPN's head backward (gfx950 / CDNA4).
//
// The RPN loss reads at most `cap` sampled anchors per image and its pair softmax couples raw channel c only with c + A of the same
// pixel, so the gradient of the head maps is exactly zero outside at most `cap` pixels per image.  The head's backward therefore runs on
// rows gathered from those pixels:
//
//   drc_srpn_active_pixels   pos | neg -> the unique active pixels of every image in ascending (level, y, x), per-image counts, and a
//                            dense index map (row or -1) over every pixel of every level
//   drc_srpn_gather_rows     T (hidden map rows), Xcol (3 x 3 x C patches of both views), G (scaled loss gradients): pure gathers
//   drc_srpn_col2im          dXcol -> the dense feature-map gradients, in gather form: every output element adds its at most nine taps
//                            in a fixed order
//
// Shapes are fixed by (N, cap): nothing is read back to the host, rows past an image's count are zero rows.  No atomics anywhere: the
// same bits run to run.  All element offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_hip.h"

namespace {

constexpr int kScanThreads = 1024;

struct LevelGeom {                      // what the kernels read of drc_srpn_levels, by value
    int32_t n_levels, N, A, C, cap;
    int32_t H[DRC_SRPN_MAX_LEVELS], W[DRC_SRPN_MAX_LEVELS];
    int64_t pix_off[DRC_SRPN_MAX_LEVELS + 1];
};

struct LevelPtrs {
    const float* left[DRC_SRPN_MAX_LEVELS];
    const float* right[DRC_SRPN_MAX_LEVELS];
    const float* hidden[DRC_SRPN_MAX_LEVELS];
    int64_t hidden_n_stride[DRC_SRPN_MAX_LEVELS];
    const float* glogits[DRC_SRPN_MAX_LEVELS];
    const float* gbbox[DRC_SRPN_MAX_LEVELS];
};

__device__ inline int level_of(const LevelGeom& g, int64_t q) {
    int l = 0;
    while (l + 1 < g.n_levels && q >= g.pix_off[l + 1]) ++l;
    return l;
}

// One block per image.  Thread t owns the pixels [t * chunk, (t + 1) * chunk): it counts its active pixels, the block scans the counts
// (exclusive, in LDS), and the thread writes its pixels' rows in order -- ascending q, the same result on every run.
__global__ __launch_bounds__(kScanThreads) void active_pixels_kernel(LevelGeom g, const uint8_t* __restrict__ pos, const uint8_t* __restrict__ neg,
                                                                     int32_t* __restrict__ row_pix, int32_t* __restrict__ counts,
                                                                     int32_t* __restrict__ index) {
    __shared__ int32_t scan[2][kScanThreads];
    const int img = blockIdx.x, t = threadIdx.x;
    const int64_t P = g.pix_off[g.n_levels];
    const int64_t chunk = (P + kScanThreads - 1) / kScanThreads;
    int64_t q0 = (int64_t)t * chunk, q1 = q0 + chunk;
    if (q0 > P) q0 = P;
    if (q1 > P) q1 = P;
    const uint8_t* mp = pos + (int64_t)img * P * g.A;
    const uint8_t* mn = neg + (int64_t)img * P * g.A;
    int32_t mine = 0;
    for (int64_t q = q0; q < q1; ++q) {
        int on = 0;
        for (int a = 0; a < g.A; ++a) on |= mp[q * g.A + a] | mn[q * g.A + a];
        mine += on ? 1 : 0;
    }
    scan[0][t] = mine;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < kScanThreads; d <<= 1) {            // Hillis-Steele inclusive scan
        const int32_t v = scan[cur][t] + (t >= d ? scan[cur][t - d] : 0);
        scan[cur ^ 1][t] = v;
        cur ^= 1;
        __syncthreads();
    }
    int32_t rank = scan[cur][t] - mine;                     // exclusive prefix of this thread
    const int32_t total = scan[cur][kScanThreads - 1];
    const int32_t kept = total < g.cap ? total : g.cap;
    for (int64_t q = q0; q < q1; ++q) {
        int on = 0;
        for (int a = 0; a < g.A; ++a) on |= mp[q * g.A + a] | mn[q * g.A + a];
        int32_t row = -1;
        if (on) {
            if (rank < g.cap) {
                row = img * g.cap + rank;
                row_pix[row] = (int32_t)q;
            }
            ++rank;
        }
        const int l = level_of(g, q);
        const int64_t hw = (int64_t)g.H[l] * g.W[l];
        index[(int64_t)g.N * g.pix_off[l] + (int64_t)img * hw + (q - g.pix_off[l])] = row;
    }
    for (int k = kept + t; k < g.cap; k += kScanThreads) row_pix[(int64_t)img * g.cap + k] = -1;
    if (t == 0) counts[img] = kept;
}

// One block per row.  A row past its image's count (row_pix < 0) is written as zeros.
__global__ __launch_bounds__(256) void gather_rows_kernel(LevelGeom g, LevelPtrs p, const int32_t* __restrict__ row_pix, const float* __restrict__ g_obj,
                                                          const float* __restrict__ g_box, float* __restrict__ T, float* __restrict__ Xcol,
                                                          float* __restrict__ G) {
    const int64_t r = blockIdx.x, rows = (int64_t)g.N * g.cap;
    const int img = (int)(r / g.cap);
    const int64_t q = row_pix[r];
    const int C = g.C, A = g.A, C4 = 4 * g.C, C9 = 9 * g.C;
    if (q < 0) {
        if (T) for (int c = threadIdx.x; c < C4; c += 256) T[r * C4 + c] = 0.f;
        if (G) for (int j = threadIdx.x; j < 8 * A; j += 256) G[r * 8 * A + j] = 0.f;
        if (Xcol) for (int j = threadIdx.x; j < C9; j += 256) {
            Xcol[r * C9 + j] = 0.f;
            Xcol[(rows + r) * C9 + j] = 0.f;
        }
        return;
    }
    const int l = level_of(g, q);
    const int H = g.H[l], W = g.W[l];
    const int64_t pix = q - g.pix_off[l], hw = (int64_t)H * W;
    const int y = (int)(pix / W), x = (int)(pix - (int64_t)y * W);
    if (T) {
        const float* hid = p.hidden[l] + (int64_t)img * p.hidden_n_stride[l] + pix * 16;
        for (int c = threadIdx.x; c < C4; c += 256) T[r * C4 + c] = hid[(int64_t)(c >> 4) * hw * 16 + (c & 15)];
    }
    if (G) {
        const float so = g_obj ? *g_obj : 0.f, sb = g_box ? *g_box : 0.f;
        const float* gz = p.glogits[l] + (int64_t)img * 2 * A * hw + pix;
        const float* gb = p.gbbox[l] + (int64_t)img * 6 * A * hw + pix;
        for (int j = threadIdx.x; j < 8 * A; j += 256)
            G[r * 8 * A + j] = j < 2 * A ? gz[(int64_t)j * hw] * so : gb[(int64_t)(j - 2 * A) * hw] * sb;
    }
    if (Xcol) {
        const float* fl = p.left[l] + (int64_t)img * C * hw;
        const float* fr = p.right[l] + (int64_t)img * C * hw;
        for (int j = threadIdx.x; j < C9; j += 256) {
            const int c = j / 9, tap = j - c * 9;
            const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
            const int64_t o = (int64_t)c * hw + (int64_t)yy * W + xx;
            Xcol[r * C9 + j] = in ? fl[o] : 0.f;
            Xcol[(rows + r) * C9 + j] = in ? fr[o] : 0.f;
        }
    }
}

// grid (pixel chunks of one level, images, views); a thread owns one pixel, looks up its nine neighbours' rows once and walks the
// channels: consecutive threads write consecutive addresses of one channel plane.
__global__ __launch_bounds__(256) void col2im_kernel(LevelGeom g, int l, float* __restrict__ dleft, float* __restrict__ dright,
                                                     const float* __restrict__ dxcol, const int32_t* __restrict__ index, int view0) {
    const int H = g.H[l], W = g.W[l], C = g.C;
    const int64_t hw = (int64_t)H * W;
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    const int img = blockIdx.y, view = view0 + blockIdx.z;
    const int y = (int)(pix / W), x = (int)(pix - (int64_t)y * W);
    const int32_t* idx = index + (int64_t)g.N * g.pix_off[l] + (int64_t)img * hw;
    const int64_t rows = (int64_t)g.N * g.cap, C9 = 9 * (int64_t)C;
    int64_t src[9];
    bool any = false;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        // the pixel whose tap (ky, kx) reads this element: (y - (ky - 1), x - (kx - 1))
        const int yy = y - (tap / 3 - 1), xx = x - (tap % 3 - 1);
        int32_t row = -1;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) row = idx[(int64_t)yy * W + xx];
        src[tap] = row < 0 ? -1 : ((int64_t)view * rows + row) * C9 + tap;
        any |= row >= 0;
    }
    float* out = (view ? dright : dleft) + (int64_t)img * C * hw + pix;
    if (!any) {
        for (int c = 0; c < C; ++c) out[(int64_t)c * hw] = 0.f;
        return;
    }
    for (int c = 0; c < C; ++c) {
        float s = 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
            if (src[tap] >= 0) s += dxcol[src[tap] + (int64_t)c * 9];
        out[(int64_t)c * hw] = s;
    }
}

int fill(const drc_srpn_levels* lv, LevelGeom* g) {
    if (!lv || lv->n_levels < 1 || lv->n_levels > DRC_SRPN_MAX_LEVELS || lv->N < 1 || lv->A < 1 || lv->C < 1 || lv->cap < 0) return -2;
    g->n_levels = lv->n_levels, g->N = lv->N, g->A = lv->A, g->C = lv->C, g->cap = lv->cap;
    int64_t off = 0;
    for (int l = 0; l < DRC_SRPN_MAX_LEVELS; ++l) {
        const bool on = l < lv->n_levels;
        if (on && (lv->H[l] < 1 || lv->W[l] < 1 || lv->pix_off[l] != off)) return -2;
        g->H[l] = on ? lv->H[l] : 1, g->W[l] = on ? lv->W[l] : 1;
        g->pix_off[l] = off;
        if (on) off += (int64_t)lv->H[l] * lv->W[l];
    }
    g->pix_off[DRC_SRPN_MAX_LEVELS] = off;
    for (int l = lv->n_levels; l <= DRC_SRPN_MAX_LEVELS; ++l) g->pix_off[l] = off;
    if (lv->pix_off[lv->n_levels] != off) return -2;
    // rows, pixels and anchors of the batch are addressed by int32 in row_pix / index / counts
    if (off * lv->A * lv->N >= (int64_t)1 << 31 || (int64_t)lv->N * lv->cap >= (int64_t)1 << 29) return -2;
    return 0;
}

}  // namespace

extern "C" {

int drc_srpn_active_pixels(const drc_srpn_levels* lv, const uint8_t* pos, const uint8_t* neg, int32_t* row_pix, int32_t* counts,
                           int32_t* index, void* stream) {
    LevelGeom g;
    const int st = fill(lv, &g);
    if (st) return st;
    if (!pos || !neg || !counts || !index || (g.cap > 0 && !row_pix)) return -1;
    hipLaunchKernelGGL(active_pixels_kernel, dim3(g.N), dim3(kScanThreads), 0, (hipStream_t)stream, g, pos, neg, row_pix, counts, index);
    return (int)hipGetLastError();
}

int drc_srpn_gather_rows(const drc_srpn_levels* lv, const int32_t* row_pix, const float* g_obj, const float* g_box, float* T, float* Xcol,
                         float* G, void* stream) {
    LevelGeom g;
    const int st = fill(lv, &g);
    if (st) return st;
    if (g.cap == 0 || (!T && !Xcol && !G)) return 0;
    if (!row_pix) return -1;
    if (T && (2 * g.C) % 16) return -2;                      // a view's hidden channels fill whole channel blocks
    LevelPtrs p;
    for (int l = 0; l < DRC_SRPN_MAX_LEVELS; ++l) {
        const bool on = l < g.n_levels;
        p.left[l] = on ? lv->left[l] : nullptr, p.right[l] = on ? lv->right[l] : nullptr;
        p.hidden[l] = on ? lv->hidden[l] : nullptr, p.hidden_n_stride[l] = on ? lv->hidden_n_stride[l] : 0;
        p.glogits[l] = on ? lv->glogits[l] : nullptr, p.gbbox[l] = on ? lv->gbbox[l] : nullptr;
        if (!on) continue;
        if ((T && (!p.hidden[l] || p.hidden_n_stride[l] < (int64_t)4 * g.C * g.H[l] * g.W[l])) || (Xcol && (!p.left[l] || !p.right[l])) ||
            (G && (!p.glogits[l] || !p.gbbox[l])))
            return -1;
    }
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)(g.N * g.cap)), dim3(256), 0, (hipStream_t)stream, g, p, row_pix, g_obj, g_box, T, Xcol, G);
    return (int)hipGetLastError();
}

int drc_srpn_col2im(const drc_srpn_levels* lv, const float* dxcol, const int32_t* index, int view_mask, void* stream) {
    LevelGeom g;
    const int st = fill(lv, &g);
    if (st) return st;
    if (view_mask < 1 || view_mask > 3) return -2;
    if (!index || (g.cap > 0 && !dxcol)) return -1;
    const int view0 = (view_mask & 1) ? 0 : 1, nviews = view_mask == 3 ? 2 : 1;
    for (int l = 0; l < g.n_levels; ++l) {
        if (((view_mask & 1) && !lv->left[l]) || ((view_mask & 2) && !lv->right[l])) return -1;
        const int64_t hw = (int64_t)g.H[l] * g.W[l];
        hipLaunchKernelGGL(col2im_kernel, dim3((unsigned)((hw + 255) / 256), g.N, nviews), dim3(256), 0, (hipStream_t)stream, g, l,
                           const_cast<float*>(lv->left[l]), const_cast<float*>(lv->right[l]), dxcol, index, view0);
    }
    return (int)hipGetLastError();
}

}  // extern "C"

// pn2_mlp.hip -- the matrix kernels of PointRCNN's RPN (gfx950): shared MLPs of the PointNet++ SA / FP modules on fp32 MFMA, and
// the proposal decode.
//
//   reference semantics: pointnet2_modules.py (QueryAndGroup -> SharedMLP -> max_pool2d; PointnetFPModule's SharedMLP),
//   pytorch_utils.py (1x1 conv + BatchNorm + ReLU, folded on the host), utils/bbox_transform.py:decode_bbox_target,
//   kitti_utils.py:boxes3d_to_bev_torch.  The schedule is ours.
//
// One body serves both matrix entry points.  A workgroup of 8 waves owns P = 32 * NCB columns (NCB = 2, 4 or 8): for the SA form a
// column is one (centroid, sample) pair, for the pointwise form one point.  out = act(W . X + b) is computed on
// v_mfma_f32_32x32x2_f32 with W as the A operand (rows = output channels) and X as the B operand (the column on the lane), so a
// layer's result has its column on the lane and its rows in the accumulator registers; ReLU(acc + b) goes to one LDS image
// H[row][column] that is the next layer's B operand.  Every layer's result is held entirely in accumulators before H is
// overwritten, so ONE hidden buffer is enough.  The first layer's input never exists as a whole: 32-row K-slices are gathered
// (xyz[idx] - centre, feats[:, idx]) into a small LDS slice, the next slice's loads in flight while the current one multiplies.
// Weights are read K-major (Wt[k][cout], prepared once by the host) straight from global memory / L2: a lane's A element for
// (row, k) is Wt[k * Cout + row], so the 32 lanes of a half-wave read 128 consecutive bytes.
//
// Work split: a "unit" is 32 output rows x 64 columns (two 32x32 accumulator tiles, 32 registers); a pass is 16 units, two per wave.
// Both units of a wave share their 64 columns, so one k-step is 2 LDS reads, 2 global reads and 4 MFMAs.  A pass covers
// 512 / 256 / 128 rows for NCB = 2 / 4 / 8; a hidden layer must fit one pass, the last layer of a chain loops over passes, and a
// single layer spreads its passes over gridDim.z (half passes, one unit per wave, when there are few workgroups).
//
// Masking.  Rows past Cout read a clamped (valid) weight address and are never stored.  K is processed in steps of 8; B rows past
// K are written as zeros (slice rows, and the rows of H up to its last 32-row block), and the A address is clamped to row K-1, so
// the products there are 0 * finite.  SA columns past `nsample` inside a centroid's power-of-two group repeat sample 0, columns of
// centroids past M repeat centroid M-1 and are not stored: a repeated column cannot change a max.  Indices are clamped to [0, N).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_pts.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMT = 512;            // threads per workgroup
constexpr int kMWaves = kMT / 64;
constexpr int kKS = 32;             // rows of a first-layer K-slice
constexpr int kUPW = 2;             // units per wave and pass

struct MlpLayer {
    const float* wt;                // [cin, cout], BN folded
    const float* bias;              // [cout]
    int cin, cout;
};

struct MlpArgs {
    // SA form
    const float* xyz;               // [B,N,3]
    const float* new_xyz;           // [B,M,3]
    const int32_t* idx;             // [B,M,ns]
    int ns, lgG;                    // group = 1 << lgG >= ns columns per centroid
    // both: in0 = feats [B,C0,N] (SA: gathered through idx), in1 [B,C1,N] (pointwise only)
    const float* in0;
    const float* in1;
    int C0, C1, N, M;               // pointwise: M == N
    float* out;                     // [B, c_total, M]
    int c_total, c_off, relu_last;
    int n_layers, hrows;
    int rbw;                        // single layer: 32-row blocks per workgroup, the passes spread over gridDim.z (0: loop over them)
    MlpLayer l[3];
};

template <int NCB>
struct Geo {
    static constexpr int P = 32 * NCB;            // columns of a workgroup
    static constexpr int NP = NCB / 2;            // 64-column pairs
    static constexpr int RPP = 16 / NP * 32;      // rows of a pass
    static constexpr int NV = kKS * P / kMT;      // slice elements per thread
};

// One slice element: row k of the first layer's input at column `col`.
template <int NCB, bool SA>
__device__ __forceinline__ float slice_elem(const MlpArgs& a, int b, int k, int col, const int* cidx, const float* ccen) {
    constexpr int P = Geo<NCB>::P;
    const int n = cidx[col];
    if (SA) {
        if (k >= a.C0 + 3) return 0.f;
        if (k < 3) return a.xyz[((int64_t)b * a.N + n) * 3 + k] - ccen[k * P + col];
        return a.in0[((int64_t)b * a.C0 + (k - 3)) * a.N + n];
    } else {
        if (k >= a.C0 + a.C1) return 0.f;
        if (k < a.C0) return a.in0[((int64_t)b * a.C0 + k) * a.N + n];
        return a.in1[((int64_t)b * a.C1 + (k - a.C0)) * a.N + n];
    }
}

template <int NCB, bool SA>
__device__ __forceinline__ void slice_load(float (&v)[Geo<NCB>::NV], const MlpArgs& a, int b, int kb, const int* cidx, const float* ccen) {
    constexpr int P = Geo<NCB>::P;
#pragma unroll
    for (int i = 0; i < Geo<NCB>::NV; ++i) {
        const int e = threadIdx.x + i * kMT;
        v[i] = slice_elem<NCB, SA>(a, b, kb + e / P, e % P, cidx, ccen);
    }
}

// acc[u][c] += W[rows of unit u][kb .. kb + rows) . Bs[0 .. rows)[columns of tile c];  rows is a multiple of 8
template <int NCB>
__device__ __forceinline__ void mma_rows(f32x16 (&acc)[kUPW][2], const MlpLayer& L, int kb, int rows, const float* Bs, const int (&rb)[kUPW],
                                         int pr, int nact) {
    constexpr int P = Geo<NCB>::P;
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const float* bp = Bs + h * P + pr * 64 + j;
    const float* ap[kUPW];
#pragma unroll
    for (int u = 0; u < kUPW; ++u) ap[u] = L.wt + min(rb[u] * 32 + j, L.cout - 1);
    const int klast = L.cin - 1;
    for (int r = 0; r < rows; r += 8) {
        float av[kUPW][4], bv[4][2];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = min(kb + r + 2 * s + h, klast);
#pragma unroll
            for (int u = 0; u < kUPW; ++u) av[u][s] = u < nact ? ap[u][(int64_t)k * L.cout] : 0.f;
            bv[s][0] = bp[(r + 2 * s) * P];
            bv[s][1] = bp[(r + 2 * s) * P + 32];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int u = 0; u < kUPW; ++u) {
                if (u < nact) {
                    acc[u][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][s], bv[s][0], acc[u][0], 0, 0, 0);
                    acc[u][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][s], bv[s][1], acc[u][1], 0, 0, 0);
                }
            }
        }
    }
}

template <int NCB, bool SA>
__global__ __launch_bounds__(kMT) void mlp_kernel(const MlpArgs a) {
    constexpr int P = Geo<NCB>::P, NP = Geo<NCB>::NP, RPP = Geo<NCB>::RPP, NV = Geo<NCB>::NV;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* H = reinterpret_cast<float*>(smem);                  // [hrows][P]
    float* S = H + (size_t)a.hrows * P;                         // [kKS][P]
    float* ccen = S + kKS * P;                                  // [3][P]
    int* cidx = reinterpret_cast<int*>(ccen + 3 * P);           // [P]
    int* cm = cidx + P;                                         // [P]: the column's centroid / point, -1 when it is not stored

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int b = blockIdx.y;
    const int G = 1 << a.lgG;

    for (int c = tid; c < P; c += kMT) {
        if (SA) {
            const int m_raw = blockIdx.x * (P >> a.lgG) + (c >> a.lgG);
            const int m = min(m_raw, a.M - 1);
            int s = c & (G - 1);
            if (s >= a.ns) s = 0;
            const int n = a.idx[((int64_t)b * a.M + m) * a.ns + s];
            cidx[c] = min(max(n, 0), a.N - 1);
            cm[c] = m_raw < a.M ? m : -1;
#pragma unroll
            for (int k = 0; k < 3; ++k) ccen[k * P + c] = a.new_xyz[((int64_t)b * a.M + m) * 3 + k];
        } else {
            const int n = blockIdx.x * P + c;
            cidx[c] = min(n, a.N - 1);
            cm[c] = n < a.N ? n : -1;
        }
    }
    __syncthreads();

    const int pr = wave % NP;
    for (int li = 0; li < a.n_layers; ++li) {
        const MlpLayer L = a.l[li];
        const bool last = li == a.n_layers - 1;
        const int npass = (last && !a.rbw) ? (L.cout + RPP - 1) / RPP : 1;
        for (int pass = 0; pass < npass; ++pass) {
            int rb[kUPW];
            int nact = 0;
#pragma unroll
            for (int u = 0; u < kUPW; ++u) {
                const int local = (wave + u * kMWaves) / NP;
                rb[u] = a.rbw ? blockIdx.z * a.rbw + local : pass * (RPP / 32) + local;
                if (rb[u] * 32 < L.cout && (!a.rbw || local < a.rbw)) nact = u + 1;
            }
            f32x16 acc[kUPW][2];
#pragma unroll
            for (int u = 0; u < kUPW; ++u)
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[u][c][r] = 0.f;

            if (li == 0) {
                float v[NV];
                slice_load<NCB, SA>(v, a, b, 0, cidx, ccen);
                for (int kb = 0; kb < L.cin; kb += kKS) {
                    __syncthreads();                            // the previous slice has been consumed
#pragma unroll
                    for (int i = 0; i < NV; ++i) S[tid + i * kMT] = v[i];
                    __syncthreads();
                    if (kb + kKS < L.cin) slice_load<NCB, SA>(v, a, b, kb + kKS, cidx, ccen);
                    const int rows = min(kKS, (L.cin - kb + 7) & ~7);
                    if (nact) mma_rows<NCB>(acc, L, kb, rows, S, rb, pr, nact);
                }
            } else {
                if (nact) mma_rows<NCB>(acc, L, 0, (L.cin + 7) & ~7, H, rb, pr, nact);
            }

            if (!last) {
                __syncthreads();                                // every wave has read this layer's input out of H
#pragma unroll
                for (int u = 0; u < kUPW; ++u) {
                    if (u < nact) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = rb[u] * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                            const float bias = L.bias[min(row, L.cout - 1)];
#pragma unroll
                            for (int c = 0; c < 2; ++c) {
                                const float x = fmaxf(acc[u][c][r] + bias, 0.f);
                                H[row * P + pr * 64 + c * 32 + j] = row < L.cout ? x : 0.f;
                            }
                        }
                    }
                }
                __syncthreads();
            } else {
#pragma unroll
                for (int u = 0; u < kUPW; ++u) {
                    if (u < nact) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = rb[u] * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                            const float bias = L.bias[min(row, L.cout - 1)];
                            float x[2];
#pragma unroll
                            for (int c = 0; c < 2; ++c) {
                                x[c] = acc[u][c][r] + bias;
                                if (a.relu_last) x[c] = fmaxf(x[c], 0.f);
                            }
                            if (SA) {
                                if (G == 64) { x[0] = fmaxf(x[0], x[1]); x[1] = x[0]; }
                                const int gl = G < 32 ? G : 32;
                                for (int o = 1; o < gl; o <<= 1) {
                                    x[0] = fmaxf(x[0], __shfl_xor(x[0], o, 64));
                                    x[1] = fmaxf(x[1], __shfl_xor(x[1], o, 64));
                                }
                                const int nc = G == 64 ? 1 : 2;
                                if ((j & (gl - 1)) == 0 && row < L.cout) {
                                    for (int c = 0; c < nc; ++c) {
                                        const int m = cm[pr * 64 + c * 32 + j];
                                        if (m >= 0) a.out[((int64_t)b * a.c_total + a.c_off + row) * a.M + m] = x[c];
                                    }
                                }
                            } else {
                                if (row < L.cout) {
#pragma unroll
                                    for (int c = 0; c < 2; ++c) {
                                        const int n = cm[pr * 64 + c * 32 + j];
                                        if (n >= 0) a.out[((int64_t)b * a.c_total + a.c_off + row) * a.M + n] = x[c];
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
    }
}

template <int NCB, bool SA>
int launch_mlp(const MlpArgs& a, int B, int cols_per_b, hipStream_t stream) {
    constexpr int P = Geo<NCB>::P;
    const size_t lds = ((size_t)a.hrows * P + (size_t)kKS * P + 3 * P) * sizeof(float) + 2 * P * sizeof(int);
    if (lds > 48 * 1024) {              // above the default limit a kernel has to opt in (a host-side call, no sync)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mlp_kernel<NCB, SA>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    const int tiles = (cols_per_b + P - 1) / P;
    MlpArgs k = a;
    int gz = 1;
    if (k.n_layers == 1) {
        // one layer: its row passes are independent, so they become workgroups; with few workgroups a wave takes one unit, not two
        const int full = Geo<NCB>::RPP / 32;
        k.rbw = ((int64_t)tiles * B < 256 && full / 2 >= kMWaves / Geo<NCB>::NP) ? full / 2 : full;
        gz = ((k.l[0].cout + 31) / 32 + k.rbw - 1) / k.rbw;
        if (gz > 65535) return -3;
    }
    hipLaunchKernelGGL((mlp_kernel<NCB, SA>), dim3(tiles, B, gz), dim3(kMT), lds, stream, k);
    return (int)hipGetLastError();
}

// the widest tile whose hidden buffer and pass size hold the layer widths; 0 when none does
int pick_ncb(int max_width, int max_hidden) {
    if (max_width <= 128 && max_hidden <= 96) return 8;
    if (max_width <= 256 && max_hidden <= 224) return 4;
    if (max_hidden <= 512) return 2;
    return 0;
}

template <bool SA>
int dispatch_mlp(MlpArgs& a, int B, int cols_per_b, void* stream) {
    int max_width = 0, max_hidden = 0;
    for (int i = 0; i < a.n_layers; ++i) {
        max_width = max_width > a.l[i].cout ? max_width : a.l[i].cout;
        if (i + 1 < a.n_layers) max_hidden = max_hidden > a.l[i].cout ? max_hidden : a.l[i].cout;
    }
    a.hrows = (max_hidden + 31) & ~31;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int ncb = pick_ncb(a.n_layers > 1 ? max_width : 0, max_hidden);     // a single layer loops over passes: any width fits
    // few columns: narrower tiles, so that more workgroups share them
    while (ncb > 2 && (int64_t)B * ((cols_per_b + 32 * ncb - 1) / (32 * ncb)) < 512) ncb >>= 1;
    switch (ncb) {
        case 8: return launch_mlp<8, SA>(a, B, cols_per_b, s);
        case 4: return launch_mlp<4, SA>(a, B, cols_per_b, s);
        case 2: return launch_mlp<2, SA>(a, B, cols_per_b, s);
    }
    return -3;
}

// ---- proposal decode: decode_bbox_target (get_y_by_bin = False, get_ry_fine = False), y += h / 2, boxes3d_to_bev
struct DecodeArgs {
    int per_loc_bin_num, num_head_bin, xz_fine, R;
    float loc_bin_size, half_bin, loc_scope, angle_per_class, half_angle, two_pi, pi, ah, aw, al;
};

__device__ __forceinline__ int first_argmax(const float* p, int n) {
    int best = 0;
    float bv = p[0];
    for (int i = 1; i < n; ++i)
        if (p[i] > bv) { bv = p[i]; best = i; }
    return best;
}

__global__ __launch_bounds__(256) void decode_kernel(int64_t total, const float* __restrict__ xyz, const float* __restrict__ reg,
                                                     float* __restrict__ boxes, float* __restrict__ bev, const DecodeArgs d) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const float* r = reg + t * d.R;
    const float* p = xyz + t * 3;
    const int nb = d.per_loc_bin_num;
    const int xb = first_argmax(r, nb), zb = first_argmax(r + nb, nb);
    float pos_x = (float)xb * d.loc_bin_size + d.half_bin - d.loc_scope;
    float pos_z = (float)zb * d.loc_bin_size + d.half_bin - d.loc_scope;
    int off = 2 * nb;
    if (d.xz_fine) {
        const float x_res = r[2 * nb + xb] * d.loc_bin_size, z_res = r[3 * nb + zb] * d.loc_bin_size;
        pos_x = pos_x + x_res;
        pos_z = pos_z + z_res;
        off = 4 * nb;
    }
    const float pos_y = p[1] + r[off];
    off += 1;
    const int rbin = first_argmax(r + off, d.num_head_bin);
    const float ry_res = r[off + d.num_head_bin + rbin] * d.half_angle;
    const float ang = (float)rbin * d.angle_per_class + ry_res;
    float ry = fmodf(ang, d.two_pi);                 // torch.remainder: fmod, then the divisor's sign
    if (ry != 0.f && ry < 0.f) ry = ry + d.two_pi;
    if (ry > d.pi) ry = ry - d.two_pi;
    off += 2 * d.num_head_bin;
    const float hh = r[off] * d.ah + d.ah, ww = r[off + 1] * d.aw + d.aw, ll = r[off + 2] * d.al + d.al;
    const float x = pos_x + p[0], z = pos_z + p[2];
    const float y = pos_y + hh / 2.f;
    float* o = boxes + t * 7;
    o[0] = x; o[1] = y; o[2] = z; o[3] = hh; o[4] = ww; o[5] = ll; o[6] = ry;
    const float half_l = ll / 2.f, half_w = ww / 2.f;
    float* e = bev + t * 5;
    e[0] = x - half_l; e[1] = z - half_w; e[2] = x + half_l; e[3] = z + half_w; e[4] = ry;
}

// |p| per point; the squares are accumulated with fused multiply-adds in x, y, z order (the rounding of torch's CPU norm reduction,
// on which the reference's recordings were made): sqrt(fma(z, z, fma(y, y, x * x)))
__global__ __launch_bounds__(256) void depth_kernel(int64_t total, const float* __restrict__ xyz, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const float x = xyz[t * 3], y = xyz[t * 3 + 1], z = xyz[t * 3 + 2];
    out[t] = sqrtf(fmaf(z, z, fmaf(y, y, x * x)));
}

}  // namespace

extern "C" {

int drc_rpn_points_depth(int64_t n, const float* xyz, float* out, void* stream) {
    if (n < 0 || !xyz || !out) return -1;
    if (n == 0) return 0;
    const int64_t blocks = (n + 255) / 256;
    if (blocks > INT32_MAX) return -2;
    hipLaunchKernelGGL(depth_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), n, xyz, out);
    return (int)hipGetLastError();
}

int drc_pn2_sa_mlp_max_fwd(int B, int N, int M, int C, int nsample, const float* xyz, const float* new_xyz, const float* feats,
                           const int32_t* idx, int n_layers, const float* wt0, const float* b0, int cout0, const float* wt1, const float* b1,
                           int cout1, const float* wt2, const float* b2, int cout2, float* out, int c_total, int c_off, void* stream) {
    if (B < 1 || N < 1 || M < 1 || C < 0 || nsample < 1 || nsample > 64 || n_layers < 1 || n_layers > 3) return -1;
    if (!xyz || !new_xyz || !idx || !out || (C > 0 && !feats)) return -1;
    const float* wt[3] = {wt0, wt1, wt2};
    const float* bs[3] = {b0, b1, b2};
    const int co[3] = {cout0, cout1, cout2};
    MlpArgs a = {};
    int cin = C + 3;
    for (int i = 0; i < n_layers; ++i) {
        if (!wt[i] || !bs[i] || co[i] < 1) return -1;
        a.l[i] = MlpLayer{wt[i], bs[i], cin, co[i]};
        cin = co[i];
    }
    if (c_off < 0 || c_off + cin > c_total || B > 65535) return -2;
    a.xyz = xyz; a.new_xyz = new_xyz; a.idx = idx; a.ns = nsample;
    a.lgG = 0;
    while ((1 << a.lgG) < nsample) ++a.lgG;
    a.in0 = feats; a.in1 = nullptr; a.C0 = C; a.C1 = 0; a.N = N; a.M = M;
    a.out = out; a.c_total = c_total; a.c_off = c_off; a.relu_last = 1; a.n_layers = n_layers;
    if ((int64_t)M << a.lgG > INT32_MAX) return -2;
    return dispatch_mlp<true>(a, B, M << a.lgG, stream);
}

int drc_pn2_pointwise_mlp_fwd(int B, int N, int C0, int C1, const float* in0, const float* in1, const float* wt, const float* bias, int cout,
                              int relu, float* out, int c_total, int c_off, void* stream) {
    if (B < 1 || N < 1 || C0 < 1 || C1 < 0 || cout < 1 || !in0 || (C1 > 0 && !in1) || !wt || !bias || !out) return -1;
    if (c_off < 0 || c_off + cout > c_total || B > 65535) return -2;
    MlpArgs a = {};
    a.in0 = in0; a.in1 = in1; a.C0 = C0; a.C1 = C1; a.N = N; a.M = N;
    a.out = out; a.c_total = c_total; a.c_off = c_off; a.relu_last = relu ? 1 : 0; a.n_layers = 1;
    a.l[0] = MlpLayer{wt, bias, C0 + C1, cout};
    return dispatch_mlp<false>(a, B, N, stream);
}

int drc_rpn_decode_proposals(int64_t n, int R, const float* xyz, const float* reg, int per_loc_bin_num, int num_head_bin, int xz_fine,
                             float loc_bin_size, float half_bin, float loc_scope, float angle_per_class, float half_angle, float two_pi,
                             float pi, float anchor_h, float anchor_w, float anchor_l, float* boxes, float* bev, void* stream) {
    if (n < 0 || per_loc_bin_num < 1 || num_head_bin < 1 || !xyz || !reg || !boxes || !bev) return -1;
    if (R != per_loc_bin_num * (xz_fine ? 4 : 2) + 1 + 2 * num_head_bin + 3) return -2;
    if (n == 0) return 0;
    const DecodeArgs d = {per_loc_bin_num, num_head_bin, xz_fine ? 1 : 0, R, loc_bin_size, half_bin, loc_scope, angle_per_class, half_angle,
                          two_pi, pi, anchor_h, anchor_w, anchor_l};
    const int64_t blocks = (n + 255) / 256;
    if (blocks > INT32_MAX) return -2;
    hipLaunchKernelGGL(decode_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), n, xyz, reg, boxes, bev, d);
    return (int)hipGetLastError();
}

}  // extern "C"

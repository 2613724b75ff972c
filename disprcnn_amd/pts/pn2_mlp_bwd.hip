// pn2_mlp_bwd.hip -- the backward of the shared MLPs of pn2_mlp.hip (gfx950): input gradient and weight / bias gradient of one
// pointwise layer on v_mfma_f32_32x32x2_f32, and the max over a neighbourhood that remembers its winner.
//
//   reference semantics: torch autograd through pytorch_utils.py's 1x1 conv (+ ReLU) and F.max_pool2d over the samples
//   (pointnet2_modules.py).  The schedule is ours.  Everything is fp32 in [B, C, N], channel-major, as the forward reads it.
//
// The layer is out = act(W . X + b), X = concat(in0, in1), W [Cout, Cin].  With gZ = gout (.) [out > 0] (gZ = gout without ReLU):
//
//   dgrad   gX[b, :, n] = W^T . gZ[b, :, n].  The forward's matrix product with W^T as the A operand: W in its own [Cout, Cin] layout
//           is the K-major form of W^T (A element (row ci, k co) = W[co * Cin + ci]), so no transpose exists.  A workgroup of 4 waves owns
//           64 columns; a wave owns one 32-row block of gX (blockIdx.z * 4 + wave) and both 32-column tiles.  32-row K-slices of gZ are
//           staged in LDS, the ReLU mask applied as the slice is loaded, the next slice's loads in flight while this one multiplies.
//           Masking as in the forward: K in steps of 8, slice rows past K are zeros, the A address is clamped to row K - 1, rows past
//           Cin read a clamped address and are never stored, columns past N read column N - 1 and are never stored.
//
//   wgrad   gW[co, ci] = sum_{b,n} gZ[b, co, n] X[b, ci, n], gb[co] = sum_{b,n} gZ[b, co, n]: the reduction runs over all B * N
//           columns, the result is tiny, so the columns are split.  A workgroup takes one chunk of kWgradChunk consecutive columns of the
//           flattened (b, n) axis and one 64 x 64 tile of the [Cout, Cin + 1] result (row Cin of X is all ones: its column is gb).  Both
//           operands have the column contiguous: 64-column pieces of 64 rows of each go through LDS with coalesced row loads
//           (leading dimension 65, so the 32 lanes of a half-wave, which read 32 rows at one column, hit 32 different banks; the two k
//           of an MFMA step are columns c and c + 32).  A piece is accumulated from zero and then added to the chunk's running sum,
//           which keeps the fp32 error of a chunk near sqrt(64) + sqrt(chunk / 64) roundings.  The partial goes to the workspace
//           [chunks][Cout][Cin + 1]; a second kernel adds the partials in fp64 in chunk order and rounds once.  No atomics: the same
//           bits run to run.
//
//   group_max  [B, C, M, ns] -> max over ns and the winner's sample index, ties to the lowest index; the backward writes every
//           element of the [B, C, M, ns] gradient (gout at the winner, zero elsewhere).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_pts.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWgradChunk = 2048;   // columns of the flattened (b, n) axis per wgrad workgroup; a multiple of kPiece
constexpr int kBT = 256;            // threads per workgroup (4 waves)
constexpr int kDP = 64;             // dgrad: columns per workgroup
constexpr int kDKS = 32;            // dgrad: rows of a K-slice
constexpr int kDNV = kDKS * kDP / kBT;
constexpr int kPiece = 64;          // wgrad: columns per LDS piece
constexpr int kLD = kPiece + 1;     // wgrad: leading dimension of a piece in LDS
constexpr int kTile = 64;           // wgrad: rows of gZ and rows of X per workgroup
constexpr int kWNV = kTile * kPiece / kBT;

struct BwdArgs {
    const float* gout;              // [B, Cout, N]
    const float* out;               // [B, Cout, N], the layer's output (read when relu)
    const float* w;                 // [Cout, Cin]
    const float* in0;               // [B, C0, N]
    const float* in1;               // [B, C1, N]
    float* gin;                     // [B, Cin, N]
    float* ws;                      // [chunks][Cout][Cin + 1]
    int B, N, C0, C1, cin, cout, relu;
    int64_t total;                  // B * N
};

// ---- dgrad
__device__ __forceinline__ float dgrad_elem(const BwdArgs& a, int b, int k, int n) {
    if (k >= a.cout) return 0.f;
    const int64_t o = ((int64_t)b * a.cout + k) * a.N + n;
    const float g = a.gout[o];
    if (a.relu) return a.out[o] > 0.f ? g : 0.f;
    return g;
}

__device__ __forceinline__ void dgrad_load(float (&v)[kDNV], const BwdArgs& a, int b, int kb, int n0) {
#pragma unroll
    for (int i = 0; i < kDNV; ++i) {
        const int e = threadIdx.x + i * kBT;
        v[i] = dgrad_elem(a, b, kb + e / kDP, min(n0 + e % kDP, a.N - 1));
    }
}

__global__ __launch_bounds__(kBT) void dgrad_kernel(const BwdArgs a) {
    __shared__ float S[kDKS * kDP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, n0 = blockIdx.x * kDP;
    const int rb = blockIdx.z * (kBT / 64) + wave;
    const bool act = rb * 32 < a.cin;                   // uniform over the wave
    f32x16 acc[2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    const float* ap = a.w + min(rb * 32 + j, a.cin - 1);
    const int klast = a.cout - 1;
    float v[kDNV];
    dgrad_load(v, a, b, 0, n0);
    for (int kb = 0; kb < a.cout; kb += kDKS) {
        __syncthreads();                                // the previous slice has been consumed
#pragma unroll
        for (int i = 0; i < kDNV; ++i) S[tid + i * kBT] = v[i];
        __syncthreads();
        if (kb + kDKS < a.cout) dgrad_load(v, a, b, kb + kDKS, n0);
        const int rows = min(kDKS, (a.cout - kb + 7) & ~7);
        if (act) {
            for (int r = 0; r < rows; r += 8) {
                float av[4], bv[4][2];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int k = min(kb + r + 2 * s + h, klast);
                    av[s] = ap[(int64_t)k * a.cin];
                    bv[s][0] = S[(r + 2 * s + h) * kDP + j];
                    bv[s][1] = S[(r + 2 * s + h) * kDP + 32 + j];
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s][0], acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s][1], acc[1], 0, 0, 0);
                }
            }
        }
    }
    if (!act) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row < a.cin) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int n = n0 + c * 32 + j;
                if (n < a.N) a.gin[((int64_t)b * a.cin + row) * a.N + n] = acc[c][r];
            }
        }
    }
}

// ---- wgrad
// column g of the flattened axis -> (b, n); a column past the end reads column total - 1 and counts as zero
__device__ __forceinline__ float wgrad_g(const BwdArgs& a, int co, int64_t g) {
    if (co >= a.cout || g >= a.total) return 0.f;
    const int b = (int)(g / a.N), n = (int)(g % a.N);
    const int64_t o = ((int64_t)b * a.cout + co) * a.N + n;
    const float v = a.gout[o];
    if (a.relu) return a.out[o] > 0.f ? v : 0.f;
    return v;
}

__device__ __forceinline__ float wgrad_x(const BwdArgs& a, int ci, int64_t g) {
    if (ci > a.cin || g >= a.total) return 0.f;
    if (ci == a.cin) return 1.f;                        // the all-ones row: its column of the result is the bias gradient
    const int b = (int)(g / a.N), n = (int)(g % a.N);
    if (ci < a.C0) return a.in0[((int64_t)b * a.C0 + ci) * a.N + n];
    return a.in1[((int64_t)b * a.C1 + (ci - a.C0)) * a.N + n];
}

__device__ __forceinline__ void wgrad_load(float (&vg)[kWNV], float (&vx)[kWNV], const BwdArgs& a, int co0, int ci0, int64_t g0) {
#pragma unroll
    for (int i = 0; i < kWNV; ++i) {
        const int e = threadIdx.x + i * kBT;
        const int row = e / kPiece;
        const int64_t g = g0 + e % kPiece;
        vg[i] = wgrad_g(a, co0 + row, g);
        vx[i] = wgrad_x(a, ci0 + row, g);
    }
}

__global__ __launch_bounds__(kBT) void wgrad_kernel(const BwdArgs a) {
    __shared__ float Gs[kTile * kLD];
    __shared__ float Xs[kTile * kLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int co0 = blockIdx.y * kTile, ci0 = blockIdx.z * kTile;
    const int64_t g_begin = (int64_t)blockIdx.x * kWgradChunk;
    const int wr = wave & 1, wc = wave >> 1;            // the wave's 32 x 32 tile of the 64 x 64 result
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float vg[kWNV], vx[kWNV];
    wgrad_load(vg, vx, a, co0, ci0, g_begin);
    for (int p = 0; p < kWgradChunk; p += kPiece) {
        if (g_begin + p >= a.total) break;              // uniform over the workgroup
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kWNV; ++i) {
            const int e = tid + i * kBT;
            Gs[(e / kPiece) * kLD + e % kPiece] = vg[i];
            Xs[(e / kPiece) * kLD + e % kPiece] = vx[i];
        }
        __syncthreads();
        if (p + kPiece < kWgradChunk) wgrad_load(vg, vx, a, co0, ci0, g_begin + p + kPiece);
        f32x16 part;
#pragma unroll
        for (int r = 0; r < 16; ++r) part[r] = 0.f;
        const float* gp = Gs + (wr * 32 + j) * kLD + 32 * h;
        const float* xp = Xs + (wc * 32 + j) * kLD + 32 * h;
#pragma unroll 8
        for (int k = 0; k < 32; ++k) part = __builtin_amdgcn_mfma_f32_32x32x2f32(gp[k], xp[k], part, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += part[r];
    }
    const int ld = a.cin + 1;
    float* dst = a.ws + (int64_t)blockIdx.x * a.cout * ld;
    const int ci = ci0 + wc * 32 + j;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = co0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (co < a.cout && ci <= a.cin) dst[(int64_t)co * ld + ci] = acc[r];
    }
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(int chunks, int cout, int cin, const float* __restrict__ ws, float* __restrict__ gw,
                                                           float* __restrict__ gb) {
    const int ld = cin + 1;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= cout * ld) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += (double)ws[(int64_t)c * cout * ld + t];
    const int co = t / ld, ci = t % ld;
    if (ci < cin) {
        if (gw) gw[(int64_t)co * cin + ci] = (float)s;
    } else if (gb) {
        gb[co] = (float)s;
    }
}

// ---- max over the neighbourhood
template <bool WITH_ARG>
__global__ __launch_bounds__(256) void group_max_fwd_kernel(int64_t rows, int ns, int lgG, const float* __restrict__ x, float* __restrict__ out,
                                                            int32_t* __restrict__ arg) {
    const int G = 1 << lgG;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row_raw = t >> lgG;
    const int s = (int)(t & (G - 1));
    const int64_t row = row_raw < rows ? row_raw : rows - 1;            // whole groups stay in the shuffles
    float v = s < ns ? x[row * ns + s] : x[row * ns];
    int i = s < ns ? s : 0;
    for (int o = 1; o < G; o <<= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    if (s == 0 && row_raw < rows) {
        out[row] = v;
        if (WITH_ARG) arg[row] = i;
    }
}

__global__ __launch_bounds__(256) void group_max_bwd_kernel(int64_t total, int ns, const float* __restrict__ gout, const int32_t* __restrict__ arg,
                                                            float* __restrict__ gin) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int64_t row = t / ns;
    const int s = (int)(t - row * ns);
    gin[t] = arg[row] == s ? gout[row] : 0.f;
}

int fill_args(BwdArgs& a, int B, int N, int C0, int C1, int cout, int relu) {
    if (B < 1 || N < 1 || C0 < 1 || C1 < 0 || cout < 1) return -1;
    if (B > 65535 || (int64_t)C0 + C1 > (1 << 20) || cout > (1 << 20)) return -2;
    a.B = B; a.N = N; a.C0 = C0; a.C1 = C1; a.cin = C0 + C1; a.cout = cout; a.relu = relu ? 1 : 0;
    a.total = (int64_t)B * N;
    return 0;
}

}  // namespace

extern "C" {

int drc_pn2_wgrad_chunk(void) { return kWgradChunk; }

int64_t drc_pn2_wgrad_workspace_floats(int B, int N, int C0, int C1, int cout) {
    if (B < 1 || N < 1 || C0 < 1 || C1 < 0 || cout < 1) return -1;
    const int64_t chunks = ((int64_t)B * N + kWgradChunk - 1) / kWgradChunk;
    return chunks * cout * ((int64_t)C0 + C1 + 1);
}

int drc_pn2_pointwise_mlp_dgrad(int B, int N, int C0, int C1, int cout, int relu, const float* gout, const float* out, const float* w,
                                float* gin, void* stream) {
    BwdArgs a = {};
    const int st = fill_args(a, B, N, C0, C1, cout, relu);
    if (st) return st;
    if (!gout || !w || !gin || (relu && !out)) return -1;
    a.gout = gout; a.out = out; a.w = w; a.gin = gin;
    const int tiles = (N + kDP - 1) / kDP;
    const int gz = ((a.cin + 31) / 32 + kBT / 64 - 1) / (kBT / 64);
    if (gz > 65535) return -2;
    hipLaunchKernelGGL(dgrad_kernel, dim3(tiles, B, gz), dim3(kBT), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

int drc_pn2_pointwise_mlp_wgrad(int B, int N, int C0, int C1, int cout, int relu, const float* gout, const float* out, const float* in0,
                                const float* in1, float* workspace, float* gw, float* gb, void* stream) {
    BwdArgs a = {};
    const int st = fill_args(a, B, N, C0, C1, cout, relu);
    if (st) return st;
    if (!gout || !in0 || (C1 > 0 && !in1) || !workspace || (!gw && !gb) || (relu && !out)) return -1;
    a.gout = gout; a.out = out; a.in0 = in0; a.in1 = in1; a.ws = workspace;
    const int64_t chunks = (a.total + kWgradChunk - 1) / kWgradChunk;
    const int ty = (cout + kTile - 1) / kTile, tz = (a.cin + 1 + kTile - 1) / kTile;
    if (chunks > INT32_MAX || ty > 65535 || tz > 65535) return -2;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(wgrad_kernel, dim3((unsigned)chunks, ty, tz), dim3(kBT), 0, s, a);
    int e = (int)hipGetLastError();
    if (e) return e;
    const int elems = cout * (a.cin + 1);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((elems + 255) / 256), dim3(256), 0, s, (int)chunks, cout, a.cin, workspace, gw, gb);
    return (int)hipGetLastError();
}

int drc_pn2_group_max_fwd(int64_t rows, int ns, const float* x, float* out, int32_t* arg, void* stream) {
    if (rows < 0 || ns < 1 || ns > 64 || !x || !out) return -1;
    if (rows == 0) return 0;
    int lgG = 0;
    while ((1 << lgG) < ns) ++lgG;
    const int64_t blocks = ((rows << lgG) + 255) / 256;
    if (blocks > INT32_MAX) return -2;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (arg)
        hipLaunchKernelGGL(group_max_fwd_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, rows, ns, lgG, x, out, arg);
    else
        hipLaunchKernelGGL(group_max_fwd_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, rows, ns, lgG, x, out, arg);
    return (int)hipGetLastError();
}

int drc_pn2_group_max_bwd(int64_t rows, int ns, const float* gout, const int32_t* arg, float* gin, void* stream) {
    if (rows < 0 || ns < 1 || ns > 64 || !gout || !arg || !gin) return -1;
    if (rows == 0) return 0;
    const int64_t total = rows * ns;
    const int64_t blocks = (total + 255) / 256;
    if (blocks > INT32_MAX) return -2;
    hipLaunchKernelGGL(group_max_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), total, ns, gout, arg, gin);
    return (int)hipGetLastError();
}

}  // extern "C"

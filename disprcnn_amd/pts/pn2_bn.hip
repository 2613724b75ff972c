// pn2_bn.hip -- BatchNorm with batch statistics for the shared MLPs of PointNet++ (gfx950): statistics, normalise + affine (+ ReLU), and
// the backward, on fp32 [B, C, N] channel-major activations, as pn2_mlp.hip writes them and pn2_mlp_bwd.hip reads them.
//
//   reference semantics: torch.nn.BatchNorm1d / BatchNorm2d in training mode followed by ReLU (pytorch_utils.py's conv -> bn -> relu), and
//   torch autograd through them.  The schedule is ours.
//
// Channel c owns B rows of N contiguous floats; its statistic runs over the n = B * N columns of the flattened (b, n) axis.  All three
// operators are bound by HBM traffic, and all of them walk the tensor the same way: a workgroup of 256 threads takes one chunk of
// kBnChunk consecutive columns of one channel (grid: chunks x C, so C = 16 with 393 k columns is 1536 workgroups), as 16-byte accesses
// when N % 4 == 0 and every base is 16-byte aligned (a group of four columns then never crosses a row), as scalar ones otherwise.  A
// thread's loads of a chunk are independent and issued together.
//
//   stats    per element, in fp64: S += y, Q += y * y (y * y is exact in fp64).  A thread adds its elements in order, the wave adds its
//            lanes in a butterfly, the first thread adds the four waves in order, and the pair goes to the workspace
//            [C][chunks][2].  A second launch, one wave per channel, adds the chunks (lane l takes chunks l, l + 64, ... in order, then
//            the butterfly), forms mean = S / n, var = Q / n - mean^2 (clamped at zero) and invstd = 1 / sqrt(var + eps) in fp64, rounds
//            each once, and updates the running statistics.  With |mean| / std = 3000 the fp64 cancellation leaves a relative 1e-9 in var.
//   apply    z = act(gamma * ((y - mean) * invstd) + beta), evaluated in fp64 from the fp32 mean / invstd and rounded once.
//   bwd      pass 1 reduces s1 = sum g, s2 = sum g * xh (g = gz masked by z > 0, xh = (y - mean) * invstd in fp64) exactly as stats does;
//            the second launch adds the chunks, leaves s1, s2 behind the partials and writes ggamma = s2, gbeta = s1; pass 2 writes
//            gy = gamma * invstd * (g - s1 / n - xh * s2 / n), in fp64, rounded once.
//
// No atomics: the same bits run to run.  The fp64 work is a handful of instructions per element, far below what the loads leave room for.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_pts.h"

namespace {

constexpr int kBnChunk = 4096;      // columns of the flattened (b, n) axis per workgroup; a multiple of 4 * kBT
constexpr int kBT = 256;            // threads per workgroup (4 waves)

struct BnArgs {
    const float* y;                 // [B, C, N]
    const float* z;                 // [B, C, N], the operator's output (bwd, read when relu)
    const float* gz;                // [B, C, N]
    const float* mi;                // [2, C]: mean, invstd
    const float* gamma;             // [C]
    const float* beta;              // [C]
    float* out;                     // [B, C, N]: z (apply) or gy (bwd)
    double* ws;                     // [C][chunks][2] partials, then [C][2] sums
    int B, C, N, relu;
    int64_t total;                  // B * N
    int chunks;
};

// Where the calling workgroup's chunk starts: the row and the column of its first element.
struct Chunk {
    int64_t g0;                     // first column of the flattened axis
    int64_t b0;                     // its row
    uint32_t n0;                    // its column within the row
};

__device__ __forceinline__ Chunk chunk_of(const BnArgs& a) {
    Chunk k;
    k.g0 = (int64_t)blockIdx.x * kBnChunk;
    k.b0 = k.g0 / a.N;
    k.n0 = (uint32_t)(k.g0 - k.b0 * a.N);
    return k;
}

// Element `off` of the chunk (off < kBnChunk) -> its index in a [B, C, N] tensor; the caller has checked g0 + off < total.
__device__ __forceinline__ int64_t index_of(const BnArgs& a, const Chunk& k, int c, int off) {
    const uint32_t m = k.n0 + (uint32_t)off;            // < N + kBnChunk <= 2^31 + 4095
    const uint32_t q = m / (uint32_t)a.N;
    const uint32_t n = m - q * (uint32_t)a.N;
    return ((k.b0 + q) * a.C + c) * (int64_t)a.N + n;
}

template <bool VEC> struct Acc {
    static constexpr int W = VEC ? 4 : 1;               // consecutive columns per access
    static constexpr int ITERS = kBnChunk / (kBT * W);  // accesses per thread and chunk
    __device__ static __forceinline__ int off(int i) { return (threadIdx.x + i * kBT) * W; }
    __device__ static __forceinline__ void load(float (&v)[W], const float* __restrict__ p, int64_t at) {
        if constexpr (VEC) {
            const float4 t = *reinterpret_cast<const float4*>(p + at);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
            v[0] = p[at];
        }
    }
    __device__ static __forceinline__ void store(float* __restrict__ p, int64_t at, const float (&v)[W]) {
        if constexpr (VEC) {
            *reinterpret_cast<float4*>(p + at) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            p[at] = v[0];
        }
    }
};

// (s, q) summed over the workgroup in a fixed order; the result is valid in thread 0.
__device__ __forceinline__ void block_sum2(double& s, double& q) {
    __shared__ double sm[2 * (kBT / 64)];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        q += __shfl_xor(q, o, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        sm[2 * wave] = s;
        sm[2 * wave + 1] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        s = sm[0];
        q = sm[1];
#pragma unroll
        for (int w = 1; w < kBT / 64; ++w) {
            s += sm[2 * w];
            q += sm[2 * w + 1];
        }
    }
}

__device__ __forceinline__ void put_partial(const BnArgs& a, int c, double s, double q) {
    if (threadIdx.x == 0) {
        double* dst = a.ws + ((int64_t)c * a.chunks + blockIdx.x) * 2;
        dst[0] = s;
        dst[1] = q;
    }
}

// ---- statistics
template <bool VEC>
__global__ __launch_bounds__(kBT) void bn_stats_kernel(const BnArgs a) {
    using A = Acc<VEC>;
    const int c = blockIdx.y;
    const Chunk k = chunk_of(a);
    float v[A::ITERS][A::W];
    bool ok[A::ITERS];
#pragma unroll
    for (int i = 0; i < A::ITERS; ++i) {
        ok[i] = k.g0 + A::off(i) < a.total;
        if (ok[i]) A::load(v[i], a.y, index_of(a, k, c, A::off(i)));
    }
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int i = 0; i < A::ITERS; ++i) {
        if (ok[i]) {
#pragma unroll
            for (int j = 0; j < A::W; ++j) {
                const double x = (double)v[i][j];
                s += x;
                q += x * x;
            }
        }
    }
    block_sum2(s, q);
    put_partial(a, c, s, q);
}

// One wave per channel: the chunks' partials added in a fixed order -> (s, q) in every lane.
__device__ __forceinline__ void sum_chunks(const BnArgs& a, int c, double& s, double& q) {
    const double* src = a.ws + (int64_t)c * a.chunks * 2;
    s = 0.0;
    q = 0.0;
    for (int j = threadIdx.x; j < a.chunks; j += 64) {
        s += src[2 * j];
        q += src[2 * j + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        q += __shfl_xor(q, o, 64);
    }
}

__global__ __launch_bounds__(64) void bn_stats_finish_kernel(const BnArgs a, float eps, float momentum, float* __restrict__ mean_invstd,
                                                             float* __restrict__ running_mean, float* __restrict__ running_var) {
    const int c = blockIdx.x;
    double s, q;
    sum_chunks(a, c, s, q);
    if (threadIdx.x != 0) return;
    const double n = (double)a.total;
    const double mean = s / n;
    double var = q / n - mean * mean;
    if (!(var > 0.0)) var = 0.0;
    mean_invstd[c] = (float)mean;
    mean_invstd[a.C + c] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) {
        const double m = (double)momentum;
        running_mean[c] = (float)((1.0 - m) * (double)running_mean[c] + m * mean);
        running_var[c] = (float)((1.0 - m) * (double)running_var[c] + m * (var * n / (n - 1.0)));
    }
}

// ---- normalise + affine (+ ReLU)
template <bool VEC>
__global__ __launch_bounds__(kBT) void bn_apply_kernel(const BnArgs a) {
    using A = Acc<VEC>;
    const int c = blockIdx.y;
    const Chunk k = chunk_of(a);
    const double mean = (double)a.mi[c], invstd = (double)a.mi[a.C + c], gamma = (double)a.gamma[c], beta = (double)a.beta[c];
    float v[A::ITERS][A::W];
    int64_t at[A::ITERS];
    bool ok[A::ITERS];
#pragma unroll
    for (int i = 0; i < A::ITERS; ++i) {
        ok[i] = k.g0 + A::off(i) < a.total;
        if (ok[i]) {
            at[i] = index_of(a, k, c, A::off(i));
            A::load(v[i], a.y, at[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < A::ITERS; ++i) {
        if (ok[i]) {
#pragma unroll
            for (int j = 0; j < A::W; ++j) {
                const float r = (float)(gamma * (((double)v[i][j] - mean) * invstd) + beta);
                v[i][j] = a.relu ? fmaxf(r, 0.f) : r;
            }
            A::store(a.out, at[i], v[i]);
        }
    }
}

// ---- backward
__device__ __forceinline__ float masked(const BnArgs& a, float gz, float z) { return a.relu ? (z > 0.f ? gz : 0.f) : gz; }

template <bool VEC>
__global__ __launch_bounds__(kBT) void bn_bwd_reduce_kernel(const BnArgs a) {
    using A = Acc<VEC>;
    const int c = blockIdx.y;
    const Chunk k = chunk_of(a);
    const double mean = (double)a.mi[c], invstd = (double)a.mi[a.C + c];
    float vg[A::ITERS][A::W], vz[A::ITERS][A::W], vy[A::ITERS][A::W];
    bool ok[A::ITERS];
#pragma unroll
    for (int i = 0; i < A::ITERS; ++i) {
        ok[i] = k.g0 + A::off(i) < a.total;
        if (ok[i]) {
            const int64_t at = index_of(a, k, c, A::off(i));
            A::load(vg[i], a.gz, at);
            A::load(vy[i], a.y, at);
            if (a.relu) A::load(vz[i], a.z, at);
        }
    }
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < A::ITERS; ++i) {
        if (ok[i]) {
#pragma unroll
            for (int j = 0; j < A::W; ++j) {
                const double g = (double)masked(a, vg[i][j], a.relu ? vz[i][j] : 0.f);
                s1 += g;
                s2 += g * (((double)vy[i][j] - mean) * invstd);
            }
        }
    }
    block_sum2(s1, s2);
    put_partial(a, c, s1, s2);
}

__global__ __launch_bounds__(64) void bn_bwd_finish_kernel(const BnArgs a, float* __restrict__ ggamma, float* __restrict__ gbeta) {
    const int c = blockIdx.x;
    double s1, s2;
    sum_chunks(a, c, s1, s2);
    if (threadIdx.x != 0) return;
    double* sums = a.ws + (int64_t)a.C * a.chunks * 2 + 2 * c;
    sums[0] = s1;
    sums[1] = s2;
    gbeta[c] = (float)s1;
    ggamma[c] = (float)s2;
}

template <bool VEC>
__global__ __launch_bounds__(kBT) void bn_bwd_apply_kernel(const BnArgs a) {
    using A = Acc<VEC>;
    const int c = blockIdx.y;
    const Chunk k = chunk_of(a);
    const double* sums = a.ws + (int64_t)a.C * a.chunks * 2 + 2 * c;
    const double n = (double)a.total;
    const double mean = (double)a.mi[c], invstd = (double)a.mi[a.C + c], scale = (double)a.gamma[c] * invstd;
    const double k1 = sums[0] / n, k2 = sums[1] / n;
    float vg[A::ITERS][A::W], vz[A::ITERS][A::W], vy[A::ITERS][A::W];
    int64_t at[A::ITERS];
    bool ok[A::ITERS];
#pragma unroll
    for (int i = 0; i < A::ITERS; ++i) {
        ok[i] = k.g0 + A::off(i) < a.total;
        if (ok[i]) {
            at[i] = index_of(a, k, c, A::off(i));
            A::load(vg[i], a.gz, at[i]);
            A::load(vy[i], a.y, at[i]);
            if (a.relu) A::load(vz[i], a.z, at[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < A::ITERS; ++i) {
        if (ok[i]) {
#pragma unroll
            for (int j = 0; j < A::W; ++j) {
                const double g = (double)masked(a, vg[i][j], a.relu ? vz[i][j] : 0.f);
                const double xh = ((double)vy[i][j] - mean) * invstd;
                vg[i][j] = (float)(scale * (g - k1 - xh * k2));
            }
            A::store(a.out, at[i], vg[i]);
        }
    }
}

int fill_args(BnArgs& a, int B, int C, int N, int relu) {
    if (B < 1 || C < 1 || N < 1 || (int64_t)B * N < 2) return -1;
    if (C > 65535) return -2;
    a.B = B; a.C = C; a.N = N; a.relu = relu ? 1 : 0;
    a.total = (int64_t)B * N;
    const int64_t chunks = (a.total + kBnChunk - 1) / kBnChunk;
    if (chunks > INT32_MAX) return -2;
    a.chunks = (int)chunks;
    return 0;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int drc_pn2_bn_chunk(void) { return kBnChunk; }

int64_t drc_pn2_bn_workspace_doubles(int B, int C, int N) {
    BnArgs a = {};
    if (fill_args(a, B, C, N, 0)) return -1;
    return 2 * (int64_t)C * ((int64_t)a.chunks + 1);
}

int drc_pn2_bn_stats(int B, int C, int N, const float* y, double* workspace, float eps, float momentum, float* mean_invstd,
                     float* running_mean, float* running_var, void* stream) {
    BnArgs a = {};
    const int st = fill_args(a, B, C, N, 0);
    if (st) return st;
    if (!y || !workspace || !mean_invstd || (running_mean == nullptr) != (running_var == nullptr)) return -1;
    a.y = y; a.ws = workspace;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(a.chunks, C);
    if (N % 4 == 0 && aligned16(y))
        hipLaunchKernelGGL(bn_stats_kernel<true>, grid, dim3(kBT), 0, s, a);
    else
        hipLaunchKernelGGL(bn_stats_kernel<false>, grid, dim3(kBT), 0, s, a);
    const int e = (int)hipGetLastError();
    if (e) return e;
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3(C), dim3(64), 0, s, a, eps, momentum, mean_invstd, running_mean, running_var);
    return (int)hipGetLastError();
}

int drc_pn2_bn_apply_fwd(int B, int C, int N, int relu, const float* y, const float* mean_invstd, const float* gamma, const float* beta,
                         float* z, void* stream) {
    BnArgs a = {};
    const int st = fill_args(a, B, C, N, relu);
    if (st) return st;
    if (!y || !mean_invstd || !gamma || !beta || !z) return -1;
    a.y = y; a.mi = mean_invstd; a.gamma = gamma; a.beta = beta; a.out = z;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(a.chunks, C);
    if (N % 4 == 0 && aligned16(y) && aligned16(z))
        hipLaunchKernelGGL(bn_apply_kernel<true>, grid, dim3(kBT), 0, s, a);
    else
        hipLaunchKernelGGL(bn_apply_kernel<false>, grid, dim3(kBT), 0, s, a);
    return (int)hipGetLastError();
}

int drc_pn2_bn_bwd(int B, int C, int N, int relu, const float* gz, const float* z, const float* y, const float* mean_invstd,
                   const float* gamma, double* workspace, float* gy, float* ggamma, float* gbeta, void* stream) {
    BnArgs a = {};
    const int st = fill_args(a, B, C, N, relu);
    if (st) return st;
    if (!gz || (relu && !z) || !y || !mean_invstd || !gamma || !workspace || !gy || !ggamma || !gbeta) return -1;
    a.gz = gz; a.z = z; a.y = y; a.mi = mean_invstd; a.gamma = gamma; a.ws = workspace; a.out = gy;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(a.chunks, C);
    const bool vec = N % 4 == 0 && aligned16(gz) && aligned16(y) && aligned16(gy) && (!relu || aligned16(z));
    if (vec)
        hipLaunchKernelGGL(bn_bwd_reduce_kernel<true>, grid, dim3(kBT), 0, s, a);
    else
        hipLaunchKernelGGL(bn_bwd_reduce_kernel<false>, grid, dim3(kBT), 0, s, a);
    int e = (int)hipGetLastError();
    if (e) return e;
    hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3(C), dim3(64), 0, s, a, ggamma, gbeta);
    e = (int)hipGetLastError();
    if (e) return e;
    if (vec)
        hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, grid, dim3(kBT), 0, s, a);
    else
        hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, grid, dim3(kBT), 0, s, a);
    return (int)hipGetLastError();
}

}  // extern "C"

// pointnet2.hip -- the PointNet++ operator set of PointRCNN (gfx950).
//
//   reference: pointnet2_lib/pointnet2/src/{sampling,ball_query,group_points,interpolate}_gpu.cu, pointnet2_api.cpp.
//
// Semantics follow the reference kernels; the schedules are ours:
//   furthest point sampling: one workgroup per batch row, up to 16 points per thread held in registers, a wave64 shuffle
//     argmax and an LDS step across the 16 waves (double-buffered: one barrier per iteration).  Ties resolve as the reference's
//     shared-memory tree does: its winner among equal distances is the slot with the smallest bit-reversed index, then the
//     first k of that slot -- a total order, so any reduction order here picks the same point.
//   ball query: one wave per centre, 64 candidates per step, ballot + prefix popcount keep the first `nsample` hits in order.
//   three_nn: LDS tiles of the known points, strict `<` insertion into double running bests, as the reference.
//   backward of gather / group / three_interpolate: no float atomics.  A per-source CSR of the index tensor (runs of a stable
//     sort) lets one thread own each source element and add its contributions in entry order: bit-identical run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_pts.h"

namespace {

constexpr int kFps = 1024;
constexpr int kFpsWaves = kFps / 64;
constexpr int kFpsPer = 16;                 // points per thread: N <= 16384
constexpr int kT = 256;
constexpr int kNnTile = 1024;

// ---- furthest point sampling
__device__ __forceinline__ uint32_t fps_key(int k, int lg) {
    const uint32_t slot = (uint32_t)k & ((1u << lg) - 1u);
    const uint32_t rev = lg ? (__builtin_bitreverse32(slot) >> (32 - lg)) : 0u;
    return (rev << 16) | ((uint32_t)k >> lg);
}

// (d1, k1) beats (d2, k2): larger distance, then the reference's tie order
__device__ __forceinline__ bool fps_better(float d1, int k1, float d2, int k2, int lg) {
    return d1 > d2 || (d1 == d2 && k1 >= 0 && (k2 < 0 || fps_key(k1, lg) < fps_key(k2, lg)));
}

__device__ __forceinline__ void fps_wave_argmax(float& d, int& k, int lg) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float od = __shfl_xor(d, o, 64);
        const int ok = __shfl_xor(k, o, 64);
        if (fps_better(od, ok, d, k, lg)) { d = od; k = ok; }
    }
}

__global__ __launch_bounds__(kFps) void fps_kernel(int n, int m, const float* __restrict__ xyz, float* __restrict__ temp,
                                                   int32_t* __restrict__ idx, int lg) {
    __shared__ float sd[2][kFpsWaves];
    __shared__ int sk[2][kFpsWaves];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* p = xyz + (int64_t)b * n * 3;
    float px[kFpsPer], py[kFpsPer], pz[kFpsPer], pt[kFpsPer];
#pragma unroll
    for (int i = 0; i < kFpsPer; ++i) {
        const int k = tid + i * kFps;
        const bool v = k < n;
        px[i] = v ? p[k * 3 + 0] : 0.f; py[i] = v ? p[k * 3 + 1] : 0.f; pz[i] = v ? p[k * 3 + 2] : 0.f;
        pt[i] = v ? temp[(int64_t)b * n + k] : 0.f;
    }
    int32_t* out = idx + (int64_t)b * m;
    int old = 0;
    if (tid == 0) out[0] = 0;
    for (int j = 1; j < m; ++j) {
        const float x1 = p[old * 3 + 0], y1 = p[old * 3 + 1], z1 = p[old * 3 + 2];
        float best = -1.f;
        int besti = -1;
#pragma unroll
        for (int i = 0; i < kFpsPer; ++i) {
            const int k = tid + i * kFps;
            if (k < n) {
                const float dx = px[i] - x1, dy = py[i] - y1, dz = pz[i] - z1;
                const float d = dx * dx + dy * dy + dz * dz;
                const float d2 = fminf(d, pt[i]);
                pt[i] = d2;
                if (fps_better(d2, k, best, besti, lg)) { best = d2; besti = k; }
            }
        }
        fps_wave_argmax(best, besti, lg);
        const int buf = j & 1;
        if (lane == 0) { sd[buf][wave] = best; sk[buf][wave] = besti; }
        __syncthreads();
        float d = lane < kFpsWaves ? sd[buf][lane] : -1.f;
        int k = lane < kFpsWaves ? sk[buf][lane] : -1;
        fps_wave_argmax(d, k, lg);                  // every wave reduces the 16 partials itself: no second barrier
        old = __shfl(k, 0, 64);
        if (tid == 0) out[j] = old;
    }
#pragma unroll
    for (int i = 0; i < kFpsPer; ++i) {
        const int k = tid + i * kFps;
        if (k < n) temp[(int64_t)b * n + k] = pt[i];
    }
}

// ---- gather / group forward
__global__ __launch_bounds__(kT) void gather_points_kernel(int C, int N, int M, const float* __restrict__ points, const int32_t* __restrict__ idx,
                                                           float* __restrict__ out, int64_t total) {
    for (int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x; t < total; t += (int64_t)gridDim.x * kT) {
        const int64_t bc = t / M;
        const int j = (int)(t - bc * M);
        const int b = (int)(bc / C);
        const int k = idx[(int64_t)b * M + j];
        out[t] = (k >= 0 && k < N) ? points[bc * N + k] : 0.f;
    }
}

__global__ __launch_bounds__(kT) void group_points_kernel(int C, int N, int K, const float* __restrict__ points, const int32_t* __restrict__ idx,
                                                          float* __restrict__ out, int64_t total) {
    for (int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x; t < total; t += (int64_t)gridDim.x * kT) {
        const int64_t bc = t / K;
        const int e = (int)(t - bc * K);
        const int b = (int)(bc / C);
        const int k = idx[(int64_t)b * K + e];
        out[t] = (k >= 0 && k < N) ? points[bc * N + k] : 0.f;
    }
}

// ---- ball query: one wave per centre
__global__ __launch_bounds__(kT) void ball_query_kernel(int B, int N, int M, float radius2, int nsample, const float* __restrict__ new_xyz,
                                                        const float* __restrict__ xyz, int32_t* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
    if (q >= (int64_t)B * M) return;
    const int b = (int)(q / M);
    const float nx = new_xyz[q * 3 + 0], ny = new_xyz[q * 3 + 1], nz = new_xyz[q * 3 + 2];
    const float* p = xyz + (int64_t)b * N * 3;
    int32_t* o = idx + q * nsample;
    int cnt = 0, first = -1;
    for (int base = 0; base < N && cnt < nsample; base += 64) {
        const int k = base + lane;
        bool hit = false;
        if (k < N) {
            const float dx = nx - p[k * 3 + 0], dy = ny - p[k * 3 + 1], dz = nz - p[k * 3 + 2];
            hit = dx * dx + dy * dy + dz * dz < radius2;
        }
        const uint64_t bal = __ballot(hit);
        if (bal == 0) continue;
        if (first < 0) first = base + __ffsll((unsigned long long)bal) - 1;
        const int pos = cnt + __popcll(bal & ((1ull << lane) - 1ull));
        if (hit && pos < nsample) o[pos] = k;
        cnt += __popcll(bal);
    }
    if (first >= 0)
        for (int l = cnt + lane; l < nsample; l += 64) o[l] = first;
}

// ---- three_nn: block of unknown points, known points staged through LDS
__global__ __launch_bounds__(kT) void three_nn_kernel(int N, int M, const float* __restrict__ unknown, const float* __restrict__ known,
                                                      float* __restrict__ dist2, int32_t* __restrict__ idx) {
    __shared__ float kx[kNnTile], ky[kNnTile], kz[kNnTile];
    const int b = blockIdx.y;
    const int i = blockIdx.x * kT + threadIdx.x;
    const bool live = i < N;
    const float* u = unknown + ((int64_t)b * N + (live ? i : 0)) * 3;
    const float ux = u[0], uy = u[1], uz = u[2];
    const float* kn = known + (int64_t)b * M * 3;
    double best1 = 1e40, best2 = 1e40, best3 = 1e40;
    int besti1 = 0, besti2 = 0, besti3 = 0;
    for (int t0 = 0; t0 < M; t0 += kNnTile) {
        const int tn = min(kNnTile, M - t0);
        __syncthreads();
        for (int t = threadIdx.x; t < tn; t += kT) {
            kx[t] = kn[(int64_t)(t0 + t) * 3 + 0]; ky[t] = kn[(int64_t)(t0 + t) * 3 + 1]; kz[t] = kn[(int64_t)(t0 + t) * 3 + 2];
        }
        __syncthreads();
        for (int t = 0; t < tn; ++t) {
            const float dx = ux - kx[t], dy = uy - ky[t], dz = uz - kz[t];
            const float d = dx * dx + dy * dy + dz * dz;
            const int k = t0 + t;
            if (d < best1) {
                best3 = best2; besti3 = besti2;
                best2 = best1; besti2 = besti1;
                best1 = d; besti1 = k;
            } else if (d < best2) {
                best3 = best2; besti3 = besti2;
                best2 = d; besti2 = k;
            } else if (d < best3) {
                best3 = d; besti3 = k;
            }
        }
    }
    if (!live) return;
    const int64_t o = ((int64_t)b * N + i) * 3;
    dist2[o + 0] = (float)best1; dist2[o + 1] = (float)best2; dist2[o + 2] = (float)best3;
    idx[o + 0] = besti1; idx[o + 1] = besti2; idx[o + 2] = besti3;
}

__global__ __launch_bounds__(kT) void three_interpolate_kernel(int C, int M, int N, const float* __restrict__ points,
                                                               const int32_t* __restrict__ idx, const float* __restrict__ weight,
                                                               float* __restrict__ out, int64_t total) {
    for (int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x; t < total; t += (int64_t)gridDim.x * kT) {
        const int64_t bc = t / N;
        const int n = (int)(t - bc * N);
        const int b = (int)(bc / C);
        const int32_t* id = idx + ((int64_t)b * N + n) * 3;
        const float* w = weight + ((int64_t)b * N + n) * 3;
        const float* pp = points + bc * M;
        const int i0 = id[0], i1 = id[1], i2 = id[2];
        const float p0 = (i0 >= 0 && i0 < M) ? pp[i0] : 0.f;
        const float p1 = (i1 >= 0 && i1 < M) ? pp[i1] : 0.f;
        const float p2 = (i2 >= 0 && i2 < M) ? pp[i2] : 0.f;
        out[t] = w[0] * p0 + w[1] * p1 + w[2] * p2;
    }
}

// ---- deterministic backward through a per-source CSR
__global__ __launch_bounds__(kT) void csr_bounds_kernel(int E, int N, const int32_t* __restrict__ keys, int32_t* __restrict__ start,
                                                        int32_t* __restrict__ end, int64_t total) {
    for (int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x; t < total; t += (int64_t)gridDim.x * kT) {
        const int64_t b = t / E;
        const int j = (int)(t - b * E);
        const int32_t* kb = keys + b * E;
        const int k = kb[j];
        if (k < 0 || k >= N) continue;
        if (j == 0 || kb[j - 1] != k) start[b * N + k] = j;
        if (j == E - 1 || kb[j + 1] != k) end[b * N + k] = j + 1;
    }
}

__global__ __launch_bounds__(kT) void csr_scatter_add_kernel(int C, int N, int K, int E, int per_col, const float* __restrict__ grad_out,
                                                             const int32_t* __restrict__ perm, const int32_t* __restrict__ start,
                                                             const int32_t* __restrict__ end, const float* __restrict__ weight,
                                                             float* __restrict__ grad_src, int64_t total) {
    for (int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x; t < total; t += (int64_t)gridDim.x * kT) {
        const int64_t bc = t / N;
        const int n = (int)(t - bc * N);
        const int64_t b = bc / C;
        const int j0 = start[b * N + n], j1 = end[b * N + n];
        const int32_t* pb = perm + b * E;
        const float* g = grad_out + bc * K;
        float s = 0.f;
        for (int j = j0; j < j1; ++j) {
            const int e = pb[j];
            float v = g[e / per_col];
            if (weight) v = weight[b * E + e] * v;
            s += v;
        }
        grad_src[t] += s;
    }
}

unsigned blocks_for(int64_t n) {
    int64_t b = (n + kT - 1) / kT;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

}  // namespace

extern "C" int drc_pn2_furthest_point_sampling(int B, int N, int M, const float* xyz, float* temp, int32_t* idx, int block_size, void* stream) {
    if (B < 0 || N < 0 || N > kFps * kFpsPer || block_size < 1 || block_size > 1024 || (block_size & (block_size - 1))) return -2;
    if (B == 0 || M <= 0) return 0;
    if (N < 1) return -2;
    if (!xyz || !temp || !idx) return -1;
    const int lg = __builtin_ctz((unsigned)block_size);
    hipLaunchKernelGGL(fps_kernel, dim3((unsigned)B), dim3(kFps), 0, (hipStream_t)stream, N, M, xyz, temp, idx, lg);
    return (int)hipGetLastError();
}

extern "C" int drc_pn2_gather_points(int B, int C, int N, int M, const float* points, const int32_t* idx, float* out, void* stream) {
    if (B < 0 || C < 0 || N < 0 || M < 0) return -2;
    const int64_t total = (int64_t)B * C * M;
    if (total == 0) return 0;
    if (!points || !idx || !out) return -1;
    hipLaunchKernelGGL(gather_points_kernel, dim3(blocks_for(total)), dim3(kT), 0, (hipStream_t)stream, C, N, M, points, idx, out, total);
    return (int)hipGetLastError();
}

extern "C" int drc_pn2_ball_query(int B, int N, int M, float radius, int nsample, const float* new_xyz, const float* xyz, int32_t* idx,
                                  void* stream) {
    if (B < 0 || N < 0 || M < 0 || nsample <= 0) return -2;
    const int64_t q = (int64_t)B * M;
    if (q == 0 || N == 0) return 0;
    if (!new_xyz || !xyz || !idx) return -1;
    const int64_t blocks = (q + kT / 64 - 1) / (kT / 64);
    if (blocks > INT32_MAX) return -2;
    hipLaunchKernelGGL(ball_query_kernel, dim3((unsigned)blocks), dim3(kT), 0, (hipStream_t)stream, B, N, M, radius * radius, nsample, new_xyz,
                       xyz, idx);
    return (int)hipGetLastError();
}

extern "C" int drc_pn2_group_points(int B, int C, int N, int M, int nsample, const float* points, const int32_t* idx, float* out, void* stream) {
    if (B < 0 || C < 0 || N < 0 || M < 0 || nsample < 0) return -2;
    const int K = M * nsample;
    const int64_t total = (int64_t)B * C * K;
    if (total == 0) return 0;
    if (!points || !idx || !out) return -1;
    hipLaunchKernelGGL(group_points_kernel, dim3(blocks_for(total)), dim3(kT), 0, (hipStream_t)stream, C, N, K, points, idx, out, total);
    return (int)hipGetLastError();
}

extern "C" int drc_pn2_three_nn(int B, int N, int M, const float* unknown, const float* known, float* dist2, int32_t* idx, void* stream) {
    if (B < 0 || N < 0 || M < 0 || B > 65535) return -2;
    if (B == 0 || N == 0) return 0;
    if (!unknown || (M > 0 && !known) || !dist2 || !idx) return -1;
    hipLaunchKernelGGL(three_nn_kernel, dim3((unsigned)((N + kT - 1) / kT), (unsigned)B), dim3(kT), 0, (hipStream_t)stream, N, M, unknown, known,
                       dist2, idx);
    return (int)hipGetLastError();
}

extern "C" int drc_pn2_three_interpolate(int B, int C, int M, int N, const float* points, const int32_t* idx, const float* weight, float* out,
                                         void* stream) {
    if (B < 0 || C < 0 || M < 0 || N < 0) return -2;
    const int64_t total = (int64_t)B * C * N;
    if (total == 0) return 0;
    if (!points || !idx || !weight || !out) return -1;
    hipLaunchKernelGGL(three_interpolate_kernel, dim3(blocks_for(total)), dim3(kT), 0, (hipStream_t)stream, C, M, N, points, idx, weight, out,
                       total);
    return (int)hipGetLastError();
}

extern "C" int drc_pn2_csr_bounds(int B, int E, int N, const int32_t* sorted_keys, int32_t* seg_start, int32_t* seg_end, void* stream) {
    if (B < 0 || E < 0 || N < 0) return -2;
    const int64_t total = (int64_t)B * E;
    if (total == 0 || N == 0) return 0;
    if (!sorted_keys || !seg_start || !seg_end) return -1;
    hipLaunchKernelGGL(csr_bounds_kernel, dim3(blocks_for(total)), dim3(kT), 0, (hipStream_t)stream, E, N, sorted_keys, seg_start, seg_end, total);
    return (int)hipGetLastError();
}

extern "C" int drc_pn2_csr_scatter_add(int B, int C, int N, int K, int E, int per_col, const float* grad_out, const int32_t* perm,
                                       const int32_t* seg_start, const int32_t* seg_end, const float* weight, float* grad_src, void* stream) {
    if (B < 0 || C < 0 || N < 0 || K < 0 || E < 0 || per_col < 1 || (int64_t)K * per_col < E) return -2;
    const int64_t total = (int64_t)B * C * N;
    if (total == 0) return 0;
    if ((E > 0 && (!grad_out || !perm)) || !seg_start || !seg_end || !grad_src) return -1;
    hipLaunchKernelGGL(csr_scatter_add_kernel, dim3(blocks_for(total)), dim3(kT), 0, (hipStream_t)stream, C, N, K, E, per_col, grad_out, perm,
                       seg_start, seg_end, weight, grad_src, total);
    return (int)hipGetLastError();
}

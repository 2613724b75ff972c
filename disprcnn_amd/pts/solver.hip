// solver.hip -- the optimizer step (gfx950): gradient norm, clipping, SGD with momentum and Adam over ALL parameter tensors at once.
//
//   reference: engine/trainer.py:110-115 (zero_grad, backward, clip_grad_norm_, optimizer.step, scheduler.step) with torch.optim.SGD / Adam
//              as solver/build.py makes them: SGD(momentum, dampening 0, no Nesterov), Adam(no amsgrad), weight decay added to the gradient.
//
// A step is three launches whatever the number of tensors: grad_norm (only when the norm is asked for), prepare (one workgroup), step.
// The host builds a work table once (disprcnn_amd/solver/fused.py) and the kernels walk it:
//   tensors int64 [T,5]: parameter pointer, gradient pointer, offset into the flat state buffers (floats, a multiple of 4), numel, group
//   chunks  int64 [C,2]: tensor, start (a multiple of kSolverChunk); a workgroup takes one chunk, a tensor without elements has none
//   hyper   fp32  [G,8]: lr, weight_decay, momentum | beta1, beta2, eps, 1 - beta1, 1 - beta2, 0.  The two complements are rounded from
//                        the host's doubles: 1 - (float)0.999 is off by 1.3e-5 of its value, which the second moment would inherit
//   derived fp32  [G,2]: Adam: lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t), evaluated in fp64 by `prepare` and rounded once
//   scalars fp32  [4]  : total_norm, clip_coef, the step count as a float (what torch keeps in state['step']), 0
//   step    int64 [1]  : the step count
// Nothing here reads back to the host, allocates or uses atomics: the learning rate is DATA (a captured graph replays with whatever the
// host last copied into `hyper`), and every sum has a fixed order, so two runs give the same bits.
//
// Alignment.  Parameters and gradients are addressed by their own pointers and only 4-byte alignment is promised: a gradient is often a
// view into one flat buffer at an arbitrary element offset.  A thread owns quads of 4 consecutive elements, the same quads whatever the
// alignment; each ARRAY of a tensor (parameter, gradient) moves a quad as one 16-byte access when its pointer is 16-byte aligned and the
// quad is whole, and element by element otherwise.  The state buffers are ours: offsets are multiples of 4 floats, so their whole quads
// are always aligned.  The arithmetic per element is the same code after either kind of load and the library builds with
// -ffp-contract=off, so the result does not depend on which path moved the data.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_pts.h"

namespace {

constexpr int kThreads = 256;
constexpr int kQuads = 4;                                  // quads per thread
constexpr int kSolverChunk = kThreads * kQuads * 4;        // 4096 elements per workgroup
constexpr int kTensorCols = 5, kChunkCols = 2, kHyperCols = 8, kDerivedCols = 2;
constexpr int kFlagNorm = 1, kFlagKeepCoef = 2, kFlagAdvance = 4;

struct Work {
    float* p;
    float* g;
    int64_t off, numel, start;
    int group;
    bool p_vec, g_vec, ok;
};

__device__ __forceinline__ Work work_of(int64_t n_tensors, int n_groups, const int64_t* tensors, const int64_t* chunks) {
    Work w = {};
    const int64_t* c = chunks + (int64_t)blockIdx.x * kChunkCols;
    const int64_t ti = c[0];
    if (ti < 0 || ti >= n_tensors) return w;               // a table that does not fit its own header: touch nothing
    const int64_t* t = tensors + ti * kTensorCols;
    w.p = reinterpret_cast<float*>(static_cast<uintptr_t>(t[0]));
    w.g = reinterpret_cast<float*>(static_cast<uintptr_t>(t[1]));
    w.off = t[2];
    w.numel = t[3];
    w.group = (int)t[4];
    w.start = c[1];
    w.p_vec = (t[0] & 15) == 0;
    w.g_vec = (t[1] & 15) == 0;
    w.ok = w.p && w.g && w.off >= 0 && (w.off & 3) == 0 && w.start >= 0 && (w.start % kSolverChunk) == 0 && w.start < w.numel &&
           w.group >= 0 && w.group < n_groups;
    return w;
}

// elements [e, e + n) of `base`, n in 1..4; the rest of v is 0
__device__ __forceinline__ void load_quad(const float* base, int64_t e, int n, bool vec, float (&v)[4]) {
    if (vec && n == 4) {
        const float4 t = *reinterpret_cast<const float4*>(base + e);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < n ? base[e + j] : 0.f;
    }
}
__device__ __forceinline__ void store_quad(float* base, int64_t e, int n, bool vec, const float (&v)[4]) {
    if (vec && n == 4) {
        *reinterpret_cast<float4*>(base + e) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) base[e + j] = v[j];
    }
}

// quad k of this thread: its first element and how many of its 4 elements the tensor has (<= 0: none)
__device__ __forceinline__ int quad_of(const Work& w, int k, int64_t& e) {
    e = w.start + ((int64_t)k * kThreads + threadIdx.x) * 4;
    const int64_t left = w.numel - e;
    return left >= 4 ? 4 : (int)left;
}

__global__ __launch_bounds__(kThreads) void grad_norm_kernel(int64_t n_tensors, const int64_t* __restrict__ tensors,
                                                             const int64_t* __restrict__ chunks, double* __restrict__ partials) {
    __shared__ double sh[kThreads];
    const Work w = work_of(n_tensors, INT32_MAX, tensors, chunks);      // the norm reads no group's constants
    double s = 0.0;
    if (w.ok) {
#pragma unroll
        for (int k = 0; k < kQuads; ++k) {
            int64_t e;
            const int n = quad_of(w, k, e);
            if (n <= 0) continue;
            float g[4];
            load_quad(w.g, e, n, w.g_vec, g);
#pragma unroll
            for (int j = 0; j < 4; ++j) s += (double)g[j] * (double)g[j];
        }
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int m = kThreads / 2; m >= 1; m >>= 1) {          // a fixed tree: thread t adds t + m
        if ((int)threadIdx.x < m) sh[threadIdx.x] += sh[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(kThreads) void prepare_kernel(int64_t n_chunks, const double* __restrict__ partials, int flags, float max_norm,
                                                           int n_groups, int adam, const float* __restrict__ hyper,
                                                           float* __restrict__ derived, float* __restrict__ scalars, int64_t* step) {
    __shared__ double sh[kThreads];
    const int tid = threadIdx.x;
    if (flags & kFlagNorm) {
        // thread t adds its run of consecutive chunks in chunk order, thread 0 adds the runs in thread order
        const int64_t per = (n_chunks + kThreads - 1) / kThreads;
        const int64_t lo = tid * per, hi = lo + per < n_chunks ? lo + per : n_chunks;
        double s = 0.0;
        for (int64_t i = lo; i < hi; ++i) s += partials[i];
        sh[tid] = s;
        __syncthreads();
        if (tid == 0) {
            double total = 0.0;
            for (int i = 0; i < kThreads; ++i) total += sh[i];
            const double norm = sqrt(total);
            const double coef = (double)max_norm / (norm + 1e-6);          // torch.nn.utils.clip_grad_norm_
            scalars[0] = (float)norm;
            scalars[1] = (float)(coef < 1.0 ? coef : 1.0);
        }
    } else if (!(flags & kFlagKeepCoef) && tid == 0) {
        scalars[1] = 1.f;
    }
    if (!(flags & kFlagAdvance)) return;
    const int64_t t = step[0] + 1;
    __syncthreads();                                       // every thread has read the old count
    if (tid == 0) {
        step[0] = t;
        scalars[2] = (float)t;
    }
    if (!adam) return;
    for (int g = tid; g < n_groups; g += kThreads) {
        const float* h = hyper + (int64_t)g * kHyperCols;
        // 1 - beta^t from 1 - beta: beta^t = exp(t * log1p(-(1 - beta)))
        const double bc1 = -expm1((double)t * log1p(-(double)h[5]));
        const double bc2 = -expm1((double)t * log1p(-(double)h[6]));
        derived[(int64_t)g * kDerivedCols + 0] = (float)((double)h[0] / bc1);
        derived[(int64_t)g * kDerivedCols + 1] = (float)(1.0 / sqrt(bc2));
    }
}

__global__ __launch_bounds__(kThreads) void sgd_step_kernel(int64_t n_tensors, int n_groups, const int64_t* __restrict__ tensors,
                                                            const int64_t* __restrict__ chunks, const float* __restrict__ hyper,
                                                            const float* __restrict__ scalars, float* __restrict__ buf, int clip) {
    const Work w = work_of(n_tensors, n_groups, tensors, chunks);
    if (!w.ok) return;
    const float* h = hyper + (int64_t)w.group * kHyperCols;
    const float lr = h[0], wd = h[1], mu = h[2];
    const float coef = clip ? scalars[1] : 1.f;
    // every load of the thread's quads first, then the arithmetic and the stores: the stores may alias the loads as far as the compiler
    // knows, so a loop over whole quads would wait for each quad's loads on its own
    int n[kQuads];
    int64_t e[kQuads];
    float p[kQuads][4], g[kQuads][4], b[kQuads][4];
#pragma unroll
    for (int k = 0; k < kQuads; ++k) {
        n[k] = quad_of(w, k, e[k]);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[k][j] = 0.f;
        if (n[k] <= 0) continue;
        load_quad(w.p, e[k], n[k], w.p_vec, p[k]);
        load_quad(w.g, e[k], n[k], w.g_vec, g[k]);
        if (buf) load_quad(buf, w.off + e[k], n[k], true, b[k]);
    }
#pragma unroll
    for (int k = 0; k < kQuads; ++k) {
        if (n[k] <= 0) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (clip) g[k][j] = g[k][j] * coef;
            const float d = g[k][j] + wd * p[k][j];
            b[k][j] = mu * b[k][j] + d;                    // a zeroed buffer makes the first step's buf = d
            p[k][j] = p[k][j] - lr * b[k][j];
        }
        if (clip) store_quad(w.g, e[k], n[k], w.g_vec, g[k]);
        if (buf) store_quad(buf, w.off + e[k], n[k], true, b[k]);
        store_quad(w.p, e[k], n[k], w.p_vec, p[k]);
    }
}

__global__ __launch_bounds__(kThreads) void adam_step_kernel(int64_t n_tensors, int n_groups, const int64_t* __restrict__ tensors,
                                                             const int64_t* __restrict__ chunks, const float* __restrict__ hyper,
                                                             const float* __restrict__ derived, const float* __restrict__ scalars,
                                                             float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq, int clip) {
    const Work w = work_of(n_tensors, n_groups, tensors, chunks);
    if (!w.ok) return;
    const float* h = hyper + (int64_t)w.group * kHyperCols;
    const float wd = h[1], beta2 = h[3], eps = h[4], w1 = h[5], w2 = h[6];
    const float step_size = derived[(int64_t)w.group * kDerivedCols + 0], inv_sqrt_bc2 = derived[(int64_t)w.group * kDerivedCols + 1];
    const float coef = clip ? scalars[1] : 1.f;
    int n[kQuads];
    int64_t e[kQuads];
    float p[kQuads][4], g[kQuads][4], m[kQuads][4], v[kQuads][4];
#pragma unroll
    for (int k = 0; k < kQuads; ++k) {                     // loads first, as in sgd_step_kernel
        n[k] = quad_of(w, k, e[k]);
        if (n[k] <= 0) continue;
        load_quad(w.p, e[k], n[k], w.p_vec, p[k]);
        load_quad(w.g, e[k], n[k], w.g_vec, g[k]);
        load_quad(exp_avg, w.off + e[k], n[k], true, m[k]);
        load_quad(exp_avg_sq, w.off + e[k], n[k], true, v[k]);
    }
#pragma unroll
    for (int k = 0; k < kQuads; ++k) {
        if (n[k] <= 0) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (clip) g[k][j] = g[k][j] * coef;
            const float d = g[k][j] + wd * p[k][j];
            m[k][j] = m[k][j] + w1 * (d - m[k][j]);
            v[k][j] = beta2 * v[k][j] + w2 * d * d;
            const float denom = sqrtf(v[k][j]) * inv_sqrt_bc2 + eps;
            p[k][j] = p[k][j] - step_size * (m[k][j] / denom);
        }
        if (clip) store_quad(w.g, e[k], n[k], w.g_vec, g[k]);
        store_quad(exp_avg, w.off + e[k], n[k], true, m[k]);
        store_quad(exp_avg_sq, w.off + e[k], n[k], true, v[k]);
        store_quad(w.p, e[k], n[k], w.p_vec, p[k]);
    }
}

inline bool grid_ok(int64_t n_chunks, int64_t n_tensors) { return n_chunks >= 0 && n_chunks <= INT32_MAX && n_tensors >= 0; }

}  // namespace

extern "C" {

int drc_solver_chunk(void) { return kSolverChunk; }

int drc_solver_grad_norm(int64_t n_chunks, int64_t n_tensors, const int64_t* tensors, const int64_t* chunks, double* partials,
                         void* stream) {
    if (!grid_ok(n_chunks, n_tensors)) return -1;
    if (n_chunks == 0) return 0;
    if (!tensors || !chunks || !partials || n_tensors < 1) return -1;
    hipLaunchKernelGGL(grad_norm_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), n_tensors, tensors,
                       chunks, partials);
    return (int)hipGetLastError();
}

int drc_solver_prepare(int64_t n_chunks, const double* partials, int flags, float max_norm, int n_groups, int adam, const float* hyper,
                       float* derived, float* scalars, int64_t* step, void* stream) {
    if (n_chunks < 0 || n_groups < 0 || !scalars || !step || (flags & ~(kFlagNorm | kFlagKeepCoef | kFlagAdvance))) return -1;
    if ((flags & kFlagNorm) && ((n_chunks > 0 && !partials) || !(max_norm >= 0.f))) return -1;
    if (adam && n_groups > 0 && (!hyper || !derived)) return -1;
    hipLaunchKernelGGL(prepare_kernel, dim3(1), dim3(kThreads), 0, static_cast<hipStream_t>(stream), n_chunks, partials, flags, max_norm,
                       n_groups, adam, hyper, derived, scalars, step);
    return (int)hipGetLastError();
}

int drc_solver_sgd_step(int64_t n_chunks, int64_t n_tensors, int n_groups, const int64_t* tensors, const int64_t* chunks,
                        const float* hyper, const float* scalars, float* momentum_buf, int clip, void* stream) {
    if (!grid_ok(n_chunks, n_tensors) || n_groups < 0) return -1;
    if (n_chunks == 0) return 0;
    if (!tensors || !chunks || !hyper || !scalars || n_tensors < 1 || n_groups < 1) return -1;
    hipLaunchKernelGGL(sgd_step_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), n_tensors, n_groups,
                       tensors, chunks, hyper, scalars, momentum_buf, clip ? 1 : 0);
    return (int)hipGetLastError();
}

int drc_solver_adam_step(int64_t n_chunks, int64_t n_tensors, int n_groups, const int64_t* tensors, const int64_t* chunks,
                         const float* hyper, const float* derived, const float* scalars, float* exp_avg, float* exp_avg_sq, int clip,
                         void* stream) {
    if (!grid_ok(n_chunks, n_tensors) || n_groups < 0) return -1;
    if (n_chunks == 0) return 0;
    if (!tensors || !chunks || !hyper || !derived || !scalars || !exp_avg || !exp_avg_sq || n_tensors < 1 || n_groups < 1) return -1;
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), n_tensors,
                       n_groups, tensors, chunks, hyper, derived, scalars, exp_avg, exp_avg_sq, clip ? 1 : 0);
    return (int)hipGetLastError();
}

}  // extern "C"

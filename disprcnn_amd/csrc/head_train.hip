// head_train.hip -- elementwise pieces of the 2D stage's head training step (gfx950 / CDNA4): the ReLU -> Dropout forward with the
// randomness as an input, and the fused activation backward + bias gradient for row-major [M][N] tensors (fully connected layers,
// predictors, the mask predictor's GEMM forms) and for the engine's blocked layout (the mask head's conv3x3 + bias + ReLU layers).
//
//   forward   y  = max(x, 0) . keep / (1 - p)           keep(m, n) = draws[m][n] >= (float)p   (nn.Dropout's distribution, not its stream)
//   backward  dz = dy . [y > 0] . keep / (1 - p)        db[n] = sum_m dz[m][n]
//
// The bias gradient is summed in fp64 in a FIXED order: every block adds its rows in row order per thread, its threads' sums in lane
// order through LDS, and writes one partial per column; a second launch adds the partials in block order.  No atomics: the same bits
// run to run.  `fold` adds f neighbouring columns into one bias entry (the 2x2 transposed convolution as a GEMM has 4 columns per output
// channel), still in fp64.  relu = 0 and p = 0 (draws = NULL) are valid forms.  All element indices are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_hip.h"

namespace {

constexpr int kCols = 64;            // columns of a row-major block (one wavefront's 256 contiguous bytes per row)
constexpr int kRowLanes = 4;         // row lanes of a block: 4 x 64 = 256 threads
constexpr int kMaxParts = 1024;      // partial sums per column the second launch walks at most

__global__ __launch_bounds__(256) void relu_dropout_fwd_kernel(const float* x, const float* __restrict__ draws, float* y, int64_t total, float p,
                                                               float scale, int relu) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        float v = x[i];
        if (relu) v = fmaxf(v, 0.f);
        if (draws) v = draws[i] >= p ? v * scale : 0.f;
        y[i] = v;
    }
}

// grid (column tiles, row blocks); block (64 columns, 4 row lanes).  Row block b owns rows [b * rows_per_block, (b + 1) * rows_per_block).
__global__ __launch_bounds__(256) void act_bwd_rows_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ draws,
                                                           float* __restrict__ dz, double* __restrict__ part, int M, int N, int rows_per_block,
                                                           float p, float scale, int relu) {
    __shared__ double red[kRowLanes][kCols];
    const int col = threadIdx.x & (kCols - 1), rl = threadIdx.x >> 6;
    const int n = blockIdx.x * kCols + col;
    const int64_t m0 = (int64_t)blockIdx.y * rows_per_block;
    int64_t m1 = m0 + rows_per_block;
    if (m1 > M) m1 = M;
    double acc = 0.0;
    if (n < N) {
        for (int64_t m = m0 + rl; m < m1; m += kRowLanes) {
            const int64_t i = m * N + n;
            float g = dy[i];
            if (relu && !(y[i] > 0.f)) g = 0.f;
            if (draws) g = draws[i] >= p ? g * scale : 0.f;
            dz[i] = g;
            acc += (double)g;
        }
    }
    if (!part) return;                                       // uniform over the grid
    red[rl][col] = acc;
    __syncthreads();
    if (rl == 0 && n < N) {
        double s = red[0][col];
#pragma unroll
        for (int j = 1; j < kRowLanes; ++j) s += red[j][col];
        part[(int64_t)blockIdx.y * N + n] = s;
    }
}

// The blocked layout float[units][CB][Hp][Wp][16] (D = 1), zero halo: dz = dy . [y > 0] on the interior (relu = 0: a copy), per-channel sums.
// grid (channel blocks, row chunks); block (16 channels, 16 pixel lanes).  Chunk b owns the rows [b * rows_per_block, ...) of the
// units * H interior rows; the three tensors share one geometry.
__global__ __launch_bounds__(256) void act_bwd_blocked_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dz,
                                                              double* __restrict__ part, int units, int CB, int H, int W, int ph, int pw,
                                                              int rows_per_block, int relu) {
    __shared__ double red[16][16];
    const int ch = threadIdx.x & 15, pl = threadIdx.x >> 4;
    const int cb = blockIdx.x;
    const int Hp = H + 2 * ph, Wp = W + 2 * pw;
    const int64_t cb_stride = (int64_t)Hp * Wp * 16, n_stride = cb_stride * CB;
    const int64_t rows = (int64_t)units * H;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    int64_t r1 = r0 + rows_per_block;
    if (r1 > rows) r1 = rows;
    const int64_t px0 = r0 * W, px1 = r1 * W;
    double acc = 0.0;
    for (int64_t q = px0 + pl; q < px1; q += 16) {
        const int64_t row = q / W;
        const int w = (int)(q - row * W);
        const int64_t u = row / H;
        const int h = (int)(row - u * H);
        const int64_t i = u * n_stride + cb * cb_stride + ((int64_t)(h + ph) * Wp + (w + pw)) * 16 + ch;
        float g = dy[i];
        if (relu && !(y[i] > 0.f)) g = 0.f;
        dz[i] = g;
        acc += (double)g;
    }
    if (!part) return;
    red[pl][ch] = acc;
    __syncthreads();
    if (pl == 0) {
        double s = red[0][ch];
#pragma unroll
        for (int j = 1; j < 16; ++j) s += red[j][ch];
        part[(int64_t)blockIdx.y * CB * 16 + cb * 16 + ch] = s;
    }
}

// db[j] = sum over the `fold` columns j * fold .. of sum over the partials in block order (fp64), rounded once to fp32
__global__ __launch_bounds__(256) void bias_partials_kernel(const double* __restrict__ part, int nparts, int N, int fold, int nout, float* __restrict__ db) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nout) return;
    double s = 0.0;
    for (int f = 0; f < fold; ++f) {
        const int n = j * fold + f;
        for (int b = 0; b < nparts; ++b) s += part[(int64_t)b * N + n];
    }
    db[j] = (float)s;
}

int rows_per_block_for(int64_t rows, int lanes) {
    int64_t per = (rows + kMaxParts - 1) / kMaxParts;
    if (per < 16 * lanes) per = 16 * lanes;
    return (int)((per + lanes - 1) / lanes * lanes);
}

}  // namespace

extern "C" {

int drc_relu_dropout_fwd(const float* x, const float* draws, float* y, int64_t total, float p, int relu, void* stream) {
    if (total < 0 || !(p >= 0.f) || !(p < 1.f)) return -2;
    if (total == 0) return 0;
    if (!x || !y || (p > 0.f && !draws)) return -1;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(relu_dropout_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, p > 0.f ? draws : nullptr, y, total, p,
                       1.f / (1.f - p), relu);
    return (int)hipGetLastError();
}

int64_t drc_act_bwd_rows_scratch_doubles(int M, int N) {
    if (M <= 0 || N <= 0) return 0;
    const int per = rows_per_block_for(M, kRowLanes);
    return (int64_t)((M + per - 1) / per) * N;
}

int drc_act_bwd_rows(const float* dy, const float* y, const float* draws, float p, int relu, int M, int N, int fold, float* dz, float* db,
                     double* scratch, int64_t scratch_doubles, void* stream) {
    if (M < 0 || N <= 0 || fold < 1 || N % fold || !(p >= 0.f) || !(p < 1.f)) return -2;
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) {
        if (db) return (int)hipMemsetAsync(db, 0, sizeof(float) * (N / fold), s);
        return 0;
    }
    if (!dy || !dz || (relu && !y) || (p > 0.f && !draws)) return -1;
    const int per = rows_per_block_for(M, kRowLanes);
    const int nparts = (M + per - 1) / per;
    if (db && (!scratch || scratch_doubles < (int64_t)nparts * N)) return -2;
    hipLaunchKernelGGL(act_bwd_rows_kernel, dim3((N + kCols - 1) / kCols, nparts), dim3(256), 0, s, dy, y, p > 0.f ? draws : nullptr, dz,
                       db ? scratch : nullptr, M, N, per, p, 1.f / (1.f - p), relu);
    if (db) {
        const int nout = N / fold;
        hipLaunchKernelGGL(bias_partials_kernel, dim3((nout + 255) / 256), dim3(256), 0, s, (const double*)scratch, nparts, N, fold, nout, db);
    }
    return (int)hipGetLastError();
}

int64_t drc_act_bwd_blocked_scratch_doubles(int units, int C, int H) {
    if (units <= 0 || C <= 0 || H <= 0) return 0;
    const int64_t rows = (int64_t)units * H;
    const int per = rows_per_block_for(rows, 1);
    return (rows + per - 1) / per * ((C + 15) / 16 * 16);
}

int drc_act_bwd_blocked(const float* dy, const float* y, int relu, int units, int C, int H, int W, int ph, int pw, float* dz, float* db,
                        double* scratch, int64_t scratch_doubles, void* stream) {
    if (units < 0 || C <= 0 || H <= 0 || W <= 0 || ph < 0 || pw < 0) return -2;
    hipStream_t s = (hipStream_t)stream;
    const int CB = (C + 15) / 16;
    if (units == 0) {
        if (db) return (int)hipMemsetAsync(db, 0, sizeof(float) * CB * 16, s);
        return 0;
    }
    if (!dy || !dz || (relu && !y)) return -1;
    const int64_t rows = (int64_t)units * H;
    const int per = rows_per_block_for(rows, 1);
    const int nparts = (int)((rows + per - 1) / per);
    if (db && (!scratch || scratch_doubles < (int64_t)nparts * CB * 16)) return -2;
    hipLaunchKernelGGL(act_bwd_blocked_kernel, dim3(CB, nparts), dim3(256), 0, s, dy, y, dz, db ? scratch : nullptr, units, CB, H, W, ph, pw, per,
                       relu);
    if (db)                                                   // db holds CB * 16 entries; those past C sum the zero padding channels
        hipLaunchKernelGGL(bias_partials_kernel, dim3((CB * 16 + 255) / 256), dim3(256), 0, s, (const double*)scratch, nparts, CB * 16, 1, CB * 16, db);
    return (int)hipGetLastError();
}

}  // extern "C"

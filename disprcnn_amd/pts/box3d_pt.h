// box3d_pt.h -- the pieces of roipool3d that boxes3d.hip, rcnn_ops.hip and proposal_target.hip share: pt_in_box3d in its mixed precision,
// the selection of the first S in-box points of one (cloud, box) by one workgroup, and the channel-major row gather of the pooled outputs.
//
//   reference: point_rcnn/lib/utils/roipool3d/src/roipool3d_kernel.cu (pt_in_box3d, get_pooled_idx)
#ifndef DISPRCNN_BOX3D_PT_H
#define DISPRCNN_BOX3D_PT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace box3d_pt {

constexpr int kPoolThreads = 256;
constexpr int kMaxPoolSamples = 8192;       // LDS index list of roipool3d: 32 KB
constexpr float kMaxDis = 10.0f;            // roipool3dLauncher's max_dis

// pt_in_box3d with its mixed precision: h / 2.0, l / 2.0, w / 2.0 are double; cos / sin of the float angle (cosa, sina)
__device__ __forceinline__ bool pt_in_box3d(float x, float y, float z, const float* bx, float cosa, float sina) {
    const float cx = bx[0], bottom_y = bx[1], cz = bx[2], h = bx[3], w = bx[4], l = bx[5];
    const float cy = (float)((double)bottom_y - (double)h / 2.0);
    if (fabsf(x - cx) > kMaxDis || (double)fabsf(y - cy) > (double)h / 2.0 || fabsf(z - cz) > kMaxDis) return false;
    const float x_rot = (x - cx) * cosa + (z - cz) * (-sina);
    const float z_rot = (x - cx) * sina + (z - cz) * cosa;
    return ((double)x_rot >= (double)(-l) / 2.0) & ((double)x_rot <= (double)l / 2.0) & ((double)z_rot >= (double)(-w) / 2.0) &
           ((double)z_rot <= (double)w / 2.0);
}

// One workgroup of kPoolThreads scans the N points p [N,3] in index order; a ballot + popcount prefix places the indices of the first S
// points inside box bx (cos / sin of bx[6] given) in sidx[0 .. min(count, S)).  -> the number of in-box points seen before the scan
// stopped (block-uniform; >= S means S were found).  wcnt: kPoolThreads / 64 ints of LDS.  Ends with a barrier.
__device__ __forceinline__ int select_in_box(int N, int S, const float* __restrict__ p, const float* bx, float cosa, float sina, int32_t* sidx,
                                             int* wcnt) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int cnt = 0;
    for (int base = 0; base < N && cnt < S; base += kPoolThreads) {
        const int k = base + tid;
        const bool in = k < N && pt_in_box3d(p[(int64_t)k * 3 + 0], p[(int64_t)k * 3 + 1], p[(int64_t)k * 3 + 2], bx, cosa, sina);
        const uint64_t bal = __ballot(in);
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kPoolThreads / 64; ++w) {
            const int c = wcnt[w];
            before += w < wave ? c : 0;
            tot += c;
        }
        const int pos = cnt + before + __popcll(bal & ((1ull << lane) - 1ull));
        if (in && pos < S) sidx[pos] = k;
        cnt += tot;
        __syncthreads();
    }
    return cnt;
}

// rows along S: out[c * S + s] = src[c * N + sidx[s]] (src null: zeros), waves take the channels in turn
__device__ __forceinline__ void gather_rows(int C, int N, int S, const float* __restrict__ src, const int32_t* sidx, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((S & 3) == 0) {
        for (int c = wave; c < C; c += kPoolThreads / 64) {
            const float* row = src ? src + (int64_t)c * N : nullptr;
            float* o = out + (int64_t)c * S;
            for (int s = lane * 4; s < S; s += 256) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row) {
                    const int4 i = *reinterpret_cast<const int4*>(sidx + s);
                    v = make_float4(row[i.x], row[i.y], row[i.z], row[i.w]);
                }
                *reinterpret_cast<float4*>(o + s) = v;
            }
        }
    } else {
        for (int c = wave; c < C; c += kPoolThreads / 64) {
            const float* row = src ? src + (int64_t)c * N : nullptr;
            float* o = out + (int64_t)c * S;
            for (int s = lane; s < S; s += 64) o[s] = row ? row[sidx[s]] : 0.f;
        }
    }
}

}  // namespace box3d_pt

#endif  // DISPRCNN_BOX3D_PT_H

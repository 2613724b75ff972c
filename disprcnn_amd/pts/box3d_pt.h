// box3d_pt.h -- the pieces of roipool3d that boxes3d.hip and rcnn_ops.hip share: pt_in_box3d in its mixed precision and the selection of
// the first S in-box points of one (cloud, box) by one workgroup.
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

}  // namespace box3d_pt

#endif  // DISPRCNN_BOX3D_PT_H

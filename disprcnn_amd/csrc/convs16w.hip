// convs16w.hip -- the cost-volume layer (dres0[0]) of the split-f16 family at large batches: two image rows per work item (rounds 6, 8).
//
//   reference arithmetic: the concat cost volume of stackhourglass.py:115-128 folded into convbn_3d 64 -> 32 k3 s1 p1 + ReLU (dres0[0],
//   :63-66,130); fp32 (config/defaults.py:22).  The arithmetic is s16_cvrows.h's (read its header first): per image row 18 2D tap maps on the
//   f16 matrix cores, every disparity plane assembled from them with adds.  convs16.hip's cost-volume form runs the same function with one row
//   per work item; the results are bit-identical (one summation order per output value).
//
// Round 6 walked the depth with two MFMA tiles per wave here (a 3D convolution over the virtual 64-channel volume: 81 MFMAs per wave, row and
// PLANE); round 8 replaced that arithmetic in both kernels.  What is left of the difference is the work item: two consecutive
// rows of a unit stay on one workgroup (the second row's three staged rows are L2 hits of the first's), half as many items to hand out.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_hip.h"
#include "s16_cvrows.h"

namespace {

constexpr int ROWS = 2;         // rows per work item
constexpr int TX = s16cv::TX;

template <int KW, bool CV>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void convs16w_kernel(const drc_s16conv_params p) {
    static_assert(CV && KW == 4, "the cost-volume layer (64 virtual input channels) is the only form");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    s16cv::s16_cvrows_run<ROWS>(p, lds);
}

template <int KW, bool CV>
int launch(const drc_s16conv_params& p, hipStream_t stream) {
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)convs16w_kernel<KW, CV>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_done = true;
    }
    hipLaunchKernelGGL((convs16w_kernel<KW, CV>), dim3((unsigned)s16cv::s16_cvrows_blocks<ROWS>(p)), dim3(256), s16cv::LDS_BYTES, stream, p);
    return (int)hipGetLastError();
}

}  // namespace

// 1 when drc_conv3d_k3_s16_fwd sends this parameter block to the two-row kernel: the cost-volume layer with whole two-row blocks and enough
// of them to give every CU several work items (smaller launches keep convs16.hip's one-row items).  Host code: no launch.
extern "C" int drc_conv3d_k3_s16_wide(const drc_s16conv_params* pp) {
    if (!pp) return 0;
    const drc_s16conv_params& p = *pp;
    const bool cv = p.left || p.right;
    if (!cv || p.res || p.y32 || p.head || !p.y16 || p.W <= 14 || p.cout != 32 || p.cin != 64) return 0;
    if (p.dil & 0x800) return 0;                              // experiment bit (`dil` is otherwise unused by the 3D layers): force the one-row kernel (A/B runs)
    if (p.H % 2) return 0;                                     // (whole row blocks only)
    const long columns = (long)p.N * (p.H / 2) * ((p.W + TX - 1) / TX);
    return columns >= 4 * 256;
}

extern "C" int drc_conv3d_k3_s16_wide_fwd(const drc_s16conv_params* pp, void* stream) {
    if (!pp) return -1;
    const drc_s16conv_params& p = *pp;
    const bool cv = p.left || p.right;
    if (!p.w || !p.scale || !p.shift || !p.y16) return -1;
    if (!cv || !p.left || !p.right || p.cin != 64) return -4;
    if (p.res || p.y32 || p.head || p.W <= 14 || p.cout != 32 || p.N < 0 || p.D <= 0 || p.H <= 0) return -4;
    if (p.N == 0) return 0;
    const long unit16 = (long)(p.cout / 32) * (p.D + 2) * (p.H + 2) * (p.W + 2) * 128;
    if (unit16 >= 0x7FFFFF00L / 2) return -5;
    return launch<4, true>(p, (hipStream_t)stream);
}

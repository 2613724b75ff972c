// mask_resize.h -- BinaryMaskList.crop / .resize of the reference (structures/segmentation_mask.py) for one ROI: the crop bounds and one pixel of
// the bilinear M x M resize, in the arithmetic of torch's CPU upsample_bilinear2d (align_corners=False).  Host and device.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace drc_mask {

struct Crop { int x0, y0, w, h; };

// round() of Python on the double of the fp32 coordinate is half-to-even: rint in the default rounding mode
__host__ __device__ inline Crop crop_bounds(const float* box, int W, int H) {
    int xmin = (int)rint((double)box[0]), ymin = (int)rint((double)box[1]), xmax = (int)rint((double)box[2]), ymax = (int)rint((double)box[3]);
    xmin = xmin < 0 ? 0 : xmin; xmin = xmin > W - 1 ? W - 1 : xmin;
    ymin = ymin < 0 ? 0 : ymin; ymin = ymin > H - 1 ? H - 1 : ymin;
    xmax = xmax < 0 ? 0 : xmax; xmax = xmax > W ? W : xmax;
    ymax = ymax < 0 ? 0 : ymax; ymax = ymax > H ? H : ymax;
    xmax = xmax > xmin + 1 ? xmax : xmin + 1;
    ymax = ymax > ymin + 1 ? ymax : ymin + 1;
    Crop c = {xmin, ymin, xmax - xmin, ymax - ymin};
    return c;
}

struct Axis { int i0, i1; float l0, l1; };

__host__ __device__ inline Axis resize_axis(int out_index, int in_size, int out_size) {
    Axis a;
    if (out_size == in_size) { a.i0 = a.i1 = out_index; a.l0 = 1.f; a.l1 = 0.f; return a; }
    const float scale = (float)in_size / (float)out_size;
    float src = fmaf(scale, (float)out_index + 0.5f, -0.5f);            // one rounding: torch's vectorised CPU kernel fuses this
    src = src < 0.f ? 0.f : src;
    int i0 = (int)floorf(src);
    i0 = i0 > in_size - 1 ? in_size - 1 : i0;
    float l1 = src - (float)i0;
    l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
    a.i0 = i0; a.i1 = i0 + (i0 < in_size - 1 ? 1 : 0); a.l1 = l1; a.l0 = 1.f - l1;
    return a;
}

// pixel (oy, ox) of the M x M resize of the crop of `mask` (row stride W); the target is 1 only where this reaches 1.0
__host__ __device__ inline float resize_pixel(const uint8_t* mask, int W, Crop c, int M, int oy, int ox) {
    const Axis ay = resize_axis(oy, c.h, M), ax = resize_axis(ox, c.w, M);
    const uint8_t* r0 = mask + (int64_t)(c.y0 + ay.i0) * W + c.x0;
    const uint8_t* r1 = mask + (int64_t)(c.y0 + ay.i1) * W + c.x0;
    // the four taps with their weights multiplied first, added left to right
    return (((float)r0[ax.i0] * (ay.l0 * ax.l0) + (float)r0[ax.i1] * (ay.l0 * ax.l1)) + (float)r1[ax.i0] * (ay.l1 * ax.l0)) +
           (float)r1[ax.i1] * (ay.l1 * ax.l1);
}

}  // namespace drc_mask

// Device functions of the pyramid operators that more than one translation unit uses: the x cells of the area-weighted resample
// (pyramid_ops.hip: resample_xy_kernel, upsample_registration_kernel; prior.hip) and one pixel of the backward registration
// (pyramid_ops.hip: registration_kernel, upsample_registration_kernel; prior.hip).  Reference-parity arithmetic: every file that
// includes this is built -ffp-contract=off, and -fno-slp-vectorize (the form of registered_value is a measured one, Makefile).
#pragma once

#include "common.hpp"

namespace {

struct ResampleXY {
    float delta_x, norm_x, delta_y, norm_y;
};

// the x cells of one output column (resample_2d.cu:46-55): worked out once per thread
struct ResampleXCells {
    int left_i, cells_x;
    float first_x, last_x;
};
__device__ __forceinline__ ResampleXCells resample_x_cells(int x, int in_w, const ResampleXY& k)
{
    const float left_f = static_cast<float>(static_cast<unsigned>(x)) * k.delta_x;
    const float right_f = static_cast<float>(static_cast<unsigned>(x) + 1u) * k.delta_x;
    ResampleXCells c;
    c.left_i = static_cast<int>(floorf(left_f));
    c.cells_x = min(in_w, static_cast<int>(ceilf(right_f))) - c.left_i;
    c.first_x = c.cells_x == 1 ? k.delta_x : static_cast<float>(c.left_i + 1) - left_f;
    c.last_x = c.cells_x == 1 ? k.delta_x : right_f - static_cast<float>(c.left_i + c.cells_x - 1);
    return c;
}

// one pixel of registration_2d.cu:34-73 (c = its offset in the planes)
__device__ __forceinline__ float registered_value(const float* __restrict__ f0, const float* __restrict__ f1, int gx, int gy, size_t c,
                                                  float uu, float vv, int w, int h, int pitch, float inv_hx, float inv_hy)
{
    const float x_f = static_cast<float>(gx) + (uu * inv_hx);
    const float y_f = static_cast<float>(gy) + (vv * inv_hy);
    if ((x_f < 0.f) || (x_f > static_cast<float>(w - 1)) || (y_f < 0.f) || (y_f > static_cast<float>(h - 1)) || isnan(x_f) ||
        isnan(y_f))
        return f0[c];
    const int x = static_cast<int>(floorf(x_f));
    const int y = static_cast<int>(floorf(y_f));
    const float dx = x_f - static_cast<float>(x);
    const float dy = y_f - static_cast<float>(y);
    const int x1 = min(w - 1, x + 1);
    const int y1 = min(h - 1, y + 1);
    // x and x1 lie in the column pair (xb, xb + 1) with xb = min(x, w - 2): each row's two values come as ONE eight-byte gather (the
    // target takes dword-aligned dwordx2 loads) instead of two -- the kernel is bound by its gathers' address processing, not by bytes
    // (round 6: registration alone 69 -> 63 us at 4096^2, the one-launch warp 23 -> 18 us at 2048^2).  (w = 1: xb = 0 and the second column is row padding, never selected.)
    const int xb = max(min(x, w - 2), 0);
    const float* r0 = f1 + static_cast<size_t>(y) * pitch + xb;
    const float* r1 = f1 + static_cast<size_t>(y1) * pitch + xb;
    const float a0 = r0[0], a1 = r0[1], b0 = r1[0], b1 = r1[1];
    const bool x_second = x != xb, x1_second = x1 != xb;
    const float r0x = x_second ? a1 : a0, r0x1 = x1_second ? a1 : a0, r1x = x_second ? b1 : b0, r1x1 = x1_second ? b1 : b0;
    return (1.f - dx) * (1.f - dy) * r0x + (dx) * (1.f - dy) * r0x1 + (1.f - dx) * (dy)*r1x + (dx) * (dy)*r1x1;
}

}  // namespace

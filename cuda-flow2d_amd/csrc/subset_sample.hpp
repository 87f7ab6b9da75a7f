// What the subset refinements that came after flow2d_subset_refine_2d share (subset_refine2.hip, subset_refine_masked.hip): a frame
// sample as a double and the Catmull-Rom sample of frame 1, as flow2d_subset_refine_2d's text in flow2d_c_abi.h states them.  Node: the
// kernel's own description of its node, of which f1, w, h and pitch (in floats) are read.
// subset_refine.hip keeps its own copy: its instruction streams are measured ones and the file is left as it is.
#pragma once

#include "plane_sample.hpp"

template <typename Offset>
__device__ __forceinline__ double sample_at(const float* f, int x, int y, int pitch)
{
    return static_cast<double>(load_at(f, pixel_offset<Offset>(x, y, pitch)));
}

// The four Catmull-Rom weights of the header for t in [0, 1).
__device__ __forceinline__ void cubic_weights(double t, double (&wt)[4])
{
    wt[0] = ((-0.5 * t + 1.0) * t - 0.5) * t;
    wt[1] = ((1.5 * t - 2.5) * t) * t + 1.0;
    wt[2] = ((-1.5 * t + 2.0) * t + 0.5) * t;
    wt[3] = ((0.5 * t - 0.5) * t) * t;
}

// g of the header at (X, Y), which lies inside [0, w - 1] x [0, h - 1].
template <typename Offset, typename Node>
__device__ __forceinline__ double cubic_sample(const Node& nd, double X, double Y)
{
    const double fx = floor(X), fy = floor(Y);
    const int ix = static_cast<int>(fx), iy = static_cast<int>(fy);
    double wx[4], wy[4];
    cubic_weights(X - fx, wx);
    cubic_weights(Y - fy, wy);
    int col[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) col[i] = min(max(ix - 1 + i, 0), nd.w - 1);
    double rows[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = min(max(iy - 1 + j, 0), nd.h - 1);
        const double a0 = sample_at<Offset>(nd.f1, col[0], y, nd.pitch), a1 = sample_at<Offset>(nd.f1, col[1], y, nd.pitch),
                     a2 = sample_at<Offset>(nd.f1, col[2], y, nd.pitch), a3 = sample_at<Offset>(nd.f1, col[3], y, nd.pitch);
        rows[j] = ((wx[0] * a0 + wx[1] * a1) + wx[2] * a2) + wx[3] * a3;
    }
    return ((wy[0] * rows[0] + wy[1] * rows[1]) + wy[2] * rows[2]) + wy[3] * rows[3];
}

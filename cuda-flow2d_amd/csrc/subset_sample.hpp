// The samples the subset refinements share (subset_refine.hip, subset_refine2.hip, subset_refine_masked.hip): a frame sample as a double and the two samples
// of the deformed frame -- the Catmull-Rom sample of frame 1, as flow2d_subset_refine_2d's text in flow2d_c_abi.h states it, and the
// cubic B-spline sample of frame 1's coefficients, as flow2d_subset_refine_spline_2d's does.  Node: the kernel's own description of
// its node (subset_node.hpp), of which f1 (the frame, or its coefficients), w, h and pitch (in floats) are read.  The kernels take
// the sample as a template parameter, CatmullRom or BSpline.
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

// The four cubic B-spline weights of the header, six times the B-spline's, for t in [0, 1).
__device__ __forceinline__ void bspline_weights(double t, double (&wt)[4])
{
    const double u = 1.0 - t;
    wt[0] = (u * u) * u;
    wt[1] = ((3.0 * t - 6.0) * t) * t + 4.0;
    wt[2] = ((3.0 * u - 6.0) * u) * u + 4.0;
    wt[3] = (t * t) * t;
}

// reflect(i, n) of flow2d_bspline_prefilter_2d's text for a tap: i in [-1, n + 1] and n >= 3 (a frame that holds a subset is three
// pixels wide at the least), so one mirroring at either end is all of it -- the smaller of |i| and its image in n - 1: four integer
// operations where the clamp of cubic_sample takes two.  twice_last = 2 (n - 1).
__device__ __forceinline__ int reflect_tap(int i, int twice_last)
{
    const int a = abs(i);
    return min(a, twice_last - a);
}

// g of flow2d_subset_refine_spline_2d at (X, Y), which lies inside [0, w - 1] x [0, h - 1]; nd.f1 holds the coefficients.
template <typename Offset, typename Node>
__device__ __forceinline__ double bspline_sample(const Node& nd, double X, double Y)
{
    const double fx = floor(X), fy = floor(Y);
    const int ix = static_cast<int>(fx), iy = static_cast<int>(fy);
    double wx[4], wy[4];
    bspline_weights(X - fx, wx);
    bspline_weights(Y - fy, wy);
    int col[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) col[i] = reflect_tap(ix - 1 + i, 2 * (nd.w - 1));
    double rows[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = reflect_tap(iy - 1 + j, 2 * (nd.h - 1));
        const double a0 = sample_at<Offset>(nd.f1, col[0], y, nd.pitch), a1 = sample_at<Offset>(nd.f1, col[1], y, nd.pitch),
                     a2 = sample_at<Offset>(nd.f1, col[2], y, nd.pitch), a3 = sample_at<Offset>(nd.f1, col[3], y, nd.pitch);
        rows[j] = ((wx[0] * a0 + wx[1] * a1) + wx[2] * a2) + wx[3] * a3;
    }
    return ((wy[0] * rows[0] + wy[1] * rows[1]) + wy[2] * rows[2]) + wy[3] * rows[3];
}

// The sample of the deformed frame as a kernel's template parameter.
struct CatmullRom {
    template <typename Offset, typename Node>
    static __device__ __forceinline__ double sample(const Node& nd, double X, double Y)
    {
        return cubic_sample<Offset>(nd, X, Y);
    }
};
struct BSpline {
    template <typename Offset, typename Node>
    static __device__ __forceinline__ double sample(const Node& nd, double X, double Y)
    {
        return bspline_sample<Offset>(nd, X, Y);
    }
};

// What the per-pixel kernels of the motion-analysis family share (consistency.hip, interpolate.hip, denoise.hip and the
// per-pixel kernels of global_motion.hip): the 64 x 4 workgroup with R rows per thread, per-lane byte offsets against scalar
// plane bases, and the bilinear sample S of flow2d_consistency_2d (flow2d_c_abi.h) read as column pairs.
//
// Two restatements of the same sample are deliberately NOT here: registered_value (pyramid_ops.hip), the reference-parity
// kernel, which is built without the SLP vectoriser and whose form is measured, and Bilinear (tracking.hip), four scalar
// gathers per track slot -- another memory pattern, whose 155 us is a measured figure.
#pragma once

#include "common.hpp"

namespace flow2d {

// Geometry: 64 x 4 threads; a thread handles column pixel_column() and the `rows` rows pixel_row(rows, i),
// one workgroup height apart, so that a wave's loads of one row are coalesced.
constexpr int kPixelBlockX = 64;
constexpr int kPixelBlockY = 4;

inline dim3 pixel_block() { return dim3(kPixelBlockX, kPixelBlockY); }
inline dim3 pixel_grid(const flow2d_context* ctx, size_t width, size_t height, int rows)
{
    return dim3(div_up(width, kPixelBlockX), div_up(div_up(height, rows), kPixelBlockY), batch_z(ctx, 1));
}

// Calls launch(Offset()) with the type of the per-lane offsets: unsigned when the largest one a lane forms -- at most
// (height - 1) * pitch + width + 1 floats, in bytes -- fits 32 bits, else size_t.  plane_bytes = height * pitch_bytes.
template <typename Launch>
void launch_by_span(size_t plane_bytes, Launch&& launch)
{
    if (plane_bytes < (size_t(1) << 32))
        launch(unsigned());
    else
        launch(size_t());
}

}  // namespace flow2d

__device__ __forceinline__ int pixel_column() { return blockIdx.x * flow2d::kPixelBlockX + threadIdx.x; }
__device__ __forceinline__ unsigned pixel_row(int rows, int i)
{
    return (blockIdx.y * rows + i) * flow2d::kPixelBlockY + threadIdx.y;
}

// Offset: unsigned (the plane's whole batch span fits 32 bits: per-lane 32-bit offsets against scalar bases) or size_t.
template <typename Offset>
__device__ __forceinline__ Offset pixel_offset(int x, int y, int pitch)
{
    return (static_cast<Offset>(y) * static_cast<Offset>(pitch) + static_cast<Offset>(x)) * sizeof(float);
}

template <typename Offset>
__device__ __forceinline__ float2 column_pair(const float* base, Offset byte_offset)
{
    const float* p = reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_offset);
    return make_float2(p[0], p[1]);
}

template <typename Offset>
__device__ __forceinline__ float load_at(const float* base, Offset byte_offset)
{
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_offset);
}

template <typename Offset>
__device__ __forceinline__ void store_at(float* base, Offset byte_offset, float value)
{
    *reinterpret_cast<float*>(reinterpret_cast<char*>(base) + byte_offset) = value;
}

// Where S(P, q) reads, for q inside [0, w - 1] x [0, h - 1].  What a kernel does with a position outside (skip the sample,
// clamp, sample at the pixel instead) is the kernel's business and happens before make_tap.
//
// The four taps are columns x = floor(qx), x1 = min(x + 1, w - 1) of rows y = floor(qy), y1 = min(y + 1, h - 1).  The column
// pair (xb, xb + 1), xb = max(min(x, w - 2), 0), holds both x and x1: one dword-aligned dwordx2 gather per row and plane, and
// one offset pair serves every plane sampled at q.  w = 1: xb = 0 and the second column is row padding (pitch >= 16 bytes),
// loaded and never selected.
template <typename Offset>
struct Tap {
    Offset o0, o1;  // byte offsets of the column pairs in rows y and y1
    float dx, dy;
    bool x_second, x1_second;  // x / x1 is the pair's second column
};

template <typename Offset>
__device__ __forceinline__ Tap<Offset> make_tap(float qx, float qy, int w, int h, int pitch)
{
    const int x = static_cast<int>(floorf(qx));
    const int y = static_cast<int>(floorf(qy));
    const int x1 = min(w - 1, x + 1);
    const int y1 = min(h - 1, y + 1);
    const int xb = max(min(x, w - 2), 0);
    Tap<Offset> t;
    t.o0 = pixel_offset<Offset>(xb, y, pitch);
    t.o1 = pixel_offset<Offset>(xb, y1, pitch);
    t.dx = qx - static_cast<float>(x);
    t.dy = qy - static_cast<float>(y);
    t.x_second = x != xb;
    t.x1_second = x1 != xb;
    return t;
}

// S from the column pairs a = column_pair(P, o0), b = column_pair(P, o1): four products, three additions, in this order.
template <typename Offset>
__device__ __forceinline__ float blend(const Tap<Offset>& t, float2 a, float2 b)
{
    const float w00 = (1.f - t.dx) * (1.f - t.dy), w01 = (t.dx) * (1.f - t.dy), w10 = (1.f - t.dx) * (t.dy), w11 = (t.dx) * (t.dy);
    return w00 * (t.x_second ? a.y : a.x) + w01 * (t.x1_second ? a.y : a.x) + w10 * (t.x_second ? b.y : b.x) +
           w11 * (t.x1_second ? b.y : b.x);
}

// Forward-backward consistency check (Sundaram, Brox & Keutzer, ECCV 2010) for gfx950: no reference counterpart.
//
// mask(x, y) = 1 where the flow (u0, v0) of frame 0 and the flow (u1, v1) of frame 1 sampled at the pixel the forward
// vector points to do not cancel, where the vector leaves the frame, or where a NaN is involved; 0 elsewhere.  The
// normative definition is the one of flow2d_consistency_2d in flow2d_c_abi.h; the bilinear sample is the operation
// order of registered_value (pyramid_ops.hip).  Built -ffp-contract=off: the bits follow that definition exactly.
//
// Memory-bound: per pixel 8 bytes of coalesced flow reads, two column-pair gathers per backward plane (the two rows the
// sample touches) and 4 bytes of mask written.  The gathers are bound by their address processing, not by bytes
// (round 6, pyramid_ops.hip): the two backward planes share the sample position, so one byte offset serves all four
// dwordx2 gathers of a pixel -- the planes' bases stay scalar and only the offset is per lane.
#include <cmath>

#include "common.hpp"

namespace {

constexpr int kBlockX = 64;
constexpr int kBlockY = 4;
constexpr int kConsistencyRows = 4;  // rows per thread: the geometry of registration_kernel

// Offset: unsigned (the planes' whole batch span fits 32 bits: per-lane 32-bit offsets against scalar bases) or size_t.
template <typename Offset>
__device__ __forceinline__ float2 column_pair(const float* __restrict__ base, Offset byte_offset)
{
    const float* p = reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_offset);
    return make_float2(p[0], p[1]);
}

template <typename Offset>
__global__ __launch_bounds__(256) void consistency_kernel(const float* __restrict__ u0, const float* __restrict__ v0,
                                                          const float* __restrict__ u1, const float* __restrict__ v1, int w,
                                                          int h, int pitch, float alpha1, float alpha2,
                                                          float* __restrict__ mask, BatchArg batch)
{
    u0 += batch_offset(batch);
    v0 += batch_offset(batch);
    u1 += batch_offset(batch);
    v1 += batch_offset(batch);
    mask += batch_offset(batch);
    const int gx = blockIdx.x * kBlockX + threadIdx.x;
    if (gx >= w) return;
    float uu[kConsistencyRows], vv[kConsistencyRows];
#pragma unroll
    for (int i = 0; i < kConsistencyRows; ++i) {
        const int gy = min((blockIdx.y * kConsistencyRows + i) * kBlockY + threadIdx.y, h - 1);
        const Offset c = static_cast<Offset>(gy) * static_cast<Offset>(pitch) + static_cast<Offset>(gx);
        uu[i] = u0[c];
        vv[i] = v0[c];
    }
    const float x_max = static_cast<float>(w - 1), y_max = static_cast<float>(h - 1);
#pragma unroll
    for (int i = 0; i < kConsistencyRows; ++i) {
        const int gy = (blockIdx.y * kConsistencyRows + i) * kBlockY + threadIdx.y;
        if (gy >= h) return;
        const Offset c = static_cast<Offset>(gy) * static_cast<Offset>(pitch) + static_cast<Offset>(gx);
        const float fu = uu[i], fv = vv[i];
        const float x_f = static_cast<float>(gx) + fu;
        const float y_f = static_cast<float>(gy) + fv;
        float out = 1.f;  // leaves the frame, or NaN
        if (x_f >= 0.f && x_f <= x_max && y_f >= 0.f && y_f <= y_max) {
            const int x = static_cast<int>(floorf(x_f));
            const int y = static_cast<int>(floorf(y_f));
            const float dx = x_f - static_cast<float>(x);
            const float dy = y_f - static_cast<float>(y);
            const int x1 = min(w - 1, x + 1);
            const int y1 = min(h - 1, y + 1);
            // the column pair (xb, xb + 1), xb = min(x, w - 2), holds x and x1: one dword-aligned dwordx2 per row and plane, as in
            // registered_value (w = 1: xb = 0 and the second column is row padding -- pitch >= 16 bytes -- never selected)
            const int xb = max(min(x, w - 2), 0);
            const Offset o0 = (static_cast<Offset>(y) * static_cast<Offset>(pitch) + static_cast<Offset>(xb)) * sizeof(float);
            const Offset o1 = (static_cast<Offset>(y1) * static_cast<Offset>(pitch) + static_cast<Offset>(xb)) * sizeof(float);
            const float2 a_u = column_pair(u1, o0), b_u = column_pair(u1, o1);
            const float2 a_v = column_pair(v1, o0), b_v = column_pair(v1, o1);
            const bool x_second = x != xb, x1_second = x1 != xb;
            const float w00 = (1.f - dx) * (1.f - dy), w01 = (dx) * (1.f - dy), w10 = (1.f - dx) * (dy), w11 = (dx) * (dy);
            const float bu = w00 * (x_second ? a_u.y : a_u.x) + w01 * (x1_second ? a_u.y : a_u.x) +
                             w10 * (x_second ? b_u.y : b_u.x) + w11 * (x1_second ? b_u.y : b_u.x);
            const float bv = w00 * (x_second ? a_v.y : a_v.x) + w01 * (x1_second ? a_v.y : a_v.x) +
                             w10 * (x_second ? b_v.y : b_v.x) + w11 * (x1_second ? b_v.y : b_v.x);
            const float eu = fu + bu, ev = fv + bv;
            const float lhs = eu * eu + ev * ev;
            const float rhs = alpha1 * ((fu * fu + fv * fv) + (bu * bu + bv * bv)) + alpha2;
            out = (lhs <= rhs) ? 0.f : 1.f;  // a NaN in the sampled flow compares false: 1
        }
        mask[c] = out;
    }
}

inline bool ranges_overlap(const void* a, const void* b, size_t bytes)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + bytes && pb < pa + bytes;
}

}  // namespace

extern "C" {

int flow2d_consistency_2d(flow2d_context* ctx, const float* flow_u, const float* flow_v, const float* back_u, const float* back_v,
                          size_t width, size_t height, size_t pitch_bytes, float alpha1, float alpha2, float* mask)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    const float* inputs[] = {flow_u, flow_v, back_u, back_v};
    for (const float* p : inputs)
        if (!flow2d::plane_args_ok(p, width, height, pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::plane_args_ok(mask, width, height, pitch_bytes) || !std::isfinite(alpha1) || !std::isfinite(alpha2) ||
        alpha1 < 0.f || alpha2 < 0.f)
        return FLOW2D_ERR_INVALID_ARGUMENT;
    // the kernel marks every plane __restrict__: the written byte range must not meet any read one (not only its base)
    for (const float* p : inputs)
        if (ranges_overlap(mask, p, height * pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    // a lock-step batch: instance b of every plane at + b * stride, so each plane spans all instances
    const size_t span = height * pitch_bytes + (ctx->batch_count - 1) * ctx->batch_stride_floats * sizeof(float);
    for (const float* p : inputs)
        if (ranges_overlap(mask, p, span)) return FLOW2D_ERR_INVALID_ARGUMENT;
    dim3 grid(flow2d::div_up(width, kBlockX), flow2d::div_up(flow2d::div_up(height, kConsistencyRows), kBlockY),
              flow2d::batch_z(ctx, 1));
    const BatchArg batch = flow2d::batch_arg(ctx, 1);
    // 32-bit per-lane offsets when the largest one a lane forms -- (height - 1) * pitch + width + 1 floats, in bytes -- fits
    if (height * pitch_bytes < (size_t(1) << 32))
        consistency_kernel<unsigned><<<grid, dim3(kBlockX, kBlockY), 0, ctx->stream>>>(
            flow_u, flow_v, back_u, back_v, (int)width, (int)height, (int)(pitch_bytes / 4), alpha1, alpha2, mask, batch);
    else
        consistency_kernel<size_t><<<grid, dim3(kBlockX, kBlockY), 0, ctx->stream>>>(
            flow_u, flow_v, back_u, back_v, (int)width, (int)height, (int)(pitch_bytes / 4), alpha1, alpha2, mask, batch);
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"

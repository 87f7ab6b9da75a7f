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

#include "plane_sample.hpp"

namespace {

constexpr int kConsistencyRows = 4;  // rows per thread: the geometry of registration_kernel

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
    const int gx = pixel_column();
    if (gx >= w) return;
    float uu[kConsistencyRows], vv[kConsistencyRows];
#pragma unroll
    for (int i = 0; i < kConsistencyRows; ++i) {
        const int gy = min(pixel_row(kConsistencyRows, i), h - 1);
        const Offset c = static_cast<Offset>(gy) * static_cast<Offset>(pitch) + static_cast<Offset>(gx);
        uu[i] = u0[c];
        vv[i] = v0[c];
    }
    const float x_max = static_cast<float>(w - 1), y_max = static_cast<float>(h - 1);
#pragma unroll
    for (int i = 0; i < kConsistencyRows; ++i) {
        const int gy = pixel_row(kConsistencyRows, i);
        if (gy >= h) return;
        const Offset c = static_cast<Offset>(gy) * static_cast<Offset>(pitch) + static_cast<Offset>(gx);
        const float fu = uu[i], fv = vv[i];
        const float x_f = static_cast<float>(gx) + fu;
        const float y_f = static_cast<float>(gy) + fv;
        float out = 1.f;  // leaves the frame, or NaN: no sample
        if (x_f >= 0.f && x_f <= x_max && y_f >= 0.f && y_f <= y_max) {
            // one offset pair serves all four gathers: the planes' bases stay scalar
            const Tap<Offset> tap = make_tap<Offset>(x_f, y_f, w, h, pitch);
            const float2 a_u = column_pair(u1, tap.o0), b_u = column_pair(u1, tap.o1);
            const float2 a_v = column_pair(v1, tap.o0), b_v = column_pair(v1, tap.o1);
            const float bu = blend(tap, a_u, b_u), bv = blend(tap, a_v, b_v);
            const float eu = fu + bu, ev = fv + bv;
            const float lhs = eu * eu + ev * ev;
            const float rhs = alpha1 * ((fu * fu + fv * fv) + (bu * bu + bv * bv)) + alpha2;
            out = (lhs <= rhs) ? 0.f : 1.f;  // a NaN in the sampled flow compares false: 1
        }
        mask[c] = out;
    }
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
    // the kernel marks every plane __restrict__: the written byte range must not meet any read one
    auto aliased = [&](size_t span) {
        const flow2d::ByteRange written[] = {{mask, span}};
        const flow2d::ByteRange read[] = {{flow_u, span}, {flow_v, span}, {back_u, span}, {back_v, span}};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(height * pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    if (aliased(flow2d::batch_span(ctx, height * pitch_bytes))) return FLOW2D_ERR_INVALID_ARGUMENT;
    flow2d::launch_by_span(height * pitch_bytes, [&](auto offset) {
        consistency_kernel<decltype(offset)><<<flow2d::pixel_grid(ctx, width, height, kConsistencyRows), flow2d::pixel_block(), 0,
                                               ctx->stream>>>(flow_u, flow_v, back_u, back_v, (int)width, (int)height,
                                                              (int)(pitch_bytes / 4), alpha1, alpha2, mask, flow2d::batch_arg(ctx, 1));
    });
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"

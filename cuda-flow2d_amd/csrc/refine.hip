// Edge-aware refinement of a flow for gfx950: a weighted median over a (2r + 1)^2 window, guided by an image, that skips
// unreliable vectors and so fills occlusions in.  No reference counterpart (the reference's post-filter is the plain median).
//
// The normative definition is the one of flow2d_refine_flow_2d in flow2d_c_abi.h.  Built -ffp-contract=off: the weights follow
// that definition bit for bit, and they are integers, so the selected value depends on no order of summation.
//
// Unlike every other analysis kernel this one is bound by the vector units and LDS, not by bytes: up to 225 samples per pixel and
// component, and a selection among them.  A workgroup of 64 x 4 threads owns a tile of 64 x 16 pixels (a thread takes four
// consecutive rows, one after the other) and stages the tile plus an r-wide halo in LDS: the order-preserving unsigned keys of
// u and v, the base weight 1 - clamp(mask) -- 0 for a sample that takes no part: outside the frame, or not a usable vector --
// and the guide.  Halo indices are clamped into the frame before they are loaded.  A thread then
//   1. computes the integer weights of its window once and keeps them in registers, two 16-bit weights per register (113
//      registers at r = 7); the window loops are unrolled, so every register index and every LDS offset is an immediate;
//   2. bisects both components at once on the key range [smallest, largest key with q > 0]: per step one pass over the window
//      that sums the weights of the keys <= the midpoint.  The loop ends when the wave's widest range is closed: a constant
//      window takes no step, a smooth one about as many as its values differ in bits, an outlier up to 32.
// Instantiated on the radius and on which of guide, mask and spatial weight are present: an absent input is neither loaded,
// staged nor multiplied in.  The record is four integer counts: per wave a butterfly, then 64-bit integer atomics (they commute:
// the same bytes in any order); the entry zeroes the record on the stream first.
// The kernel is refine_kernel.hpp; this file holds the entry.
#include "refine_kernel.hpp"

void flow2d_refine_launch_r1(flow2d_context*, const RefineArgs&, bool, size_t, size_t);
void flow2d_refine_launch_r2(flow2d_context*, const RefineArgs&, bool, size_t, size_t);
void flow2d_refine_launch_r3(flow2d_context*, const RefineArgs&, bool, size_t, size_t);
void flow2d_refine_launch_r4(flow2d_context*, const RefineArgs&, bool, size_t, size_t);
void flow2d_refine_launch_r5(flow2d_context*, const RefineArgs&, bool, size_t, size_t);
void flow2d_refine_launch_r6(flow2d_context*, const RefineArgs&, bool, size_t, size_t);
void flow2d_refine_launch_r7(flow2d_context*, const RefineArgs&, bool, size_t, size_t);

namespace {
constexpr RefineLaunch kLaunch[FLOW2D_REFINE_MAX_RADIUS] = {flow2d_refine_launch_r1, flow2d_refine_launch_r2, flow2d_refine_launch_r3,
                                                            flow2d_refine_launch_r4, flow2d_refine_launch_r5, flow2d_refine_launch_r6,
                                                            flow2d_refine_launch_r7};
}

extern "C" {

int flow2d_refine_flow_2d(flow2d_context* ctx, const float* flow_u, const float* flow_v, const float* guide, const float* mask,
                          size_t width, size_t height, size_t pitch_bytes, int radius, float sigma_guide, float sigma_space,
                          float* out_u, float* out_v, flow2d_refine_record* record)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    if (!flow2d::plane_args_ok(flow_u, width, height, pitch_bytes) || !flow2d::plane_args_ok(flow_v, width, height, pitch_bytes) ||
        !flow2d::plane_args_ok(out_u, width, height, pitch_bytes) || !flow2d::plane_args_ok(out_v, width, height, pitch_bytes) ||
        (guide && !flow2d::plane_args_ok(guide, width, height, pitch_bytes)) ||
        (mask && !flow2d::plane_args_ok(mask, width, height, pitch_bytes)))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (radius < 1 || radius > FLOW2D_REFINE_MAX_RADIUS) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!(sigma_guide >= 0.f) || !(sigma_space >= 0.f) || std::isinf(sigma_guide) || std::isinf(sigma_space))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if ((reinterpret_cast<uintptr_t>(record) % alignof(flow2d_refine_record)) != 0) return FLOW2D_ERR_INVALID_ARGUMENT;
    // the kernel marks every plane it reads __restrict__ and reads a window of them: no written byte range may meet a read one
    // or another written one
    auto aliased = [&](size_t span, size_t instances) {
        const flow2d::ByteRange written[] = {{out_u, span}, {out_v, span}, {record, instances * sizeof(flow2d_refine_record)}};
        const flow2d::ByteRange read[] = {{flow_u, span}, {flow_v, span}, {guide, span}, {mask, span}};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(height * pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t instances = ctx->batch_count;
    if (aliased(flow2d::batch_span(ctx, height * pitch_bytes), instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (record) FLOW2D_HIP_TRY(hipMemsetAsync(record, 0, instances * sizeof(flow2d_refine_record), ctx->stream));
    // a guide with sigma_guide = 0 is no guide, a sigma_space of 0 no spatial weight
    const RefineArgs a = {flow_u, flow_v, sigma_guide > 0.f ? guide : nullptr, mask, out_u, out_v,
                          reinterpret_cast<unsigned long long*>(record), static_cast<int>(width), static_cast<int>(height),
                          static_cast<int>(pitch_bytes / 4), sigma_guide * sigma_guide, sigma_space * sigma_space, sigma_space > 0.f};
    // (the largest offset a lane forms is below height * pitch_bytes)
    flow2d::launch_by_span(height * pitch_bytes, [&](auto offset) {
        kLaunch[radius - 1](ctx, a, sizeof(decltype(offset)) > 4, width, height);
    });
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"

// What the subset refinements of order 1 and 2 share beside the samplers of subset_sample.hpp (subset_refine.hip,
// subset_refine_masked.hip, subset_refine2.hip): the states, the limits of a workgroup, the common part of a wave's node, the frame-0 quantities, the
// frame-0 window test, and the one host body of their entries.  The definitions restated are those of flow2d_subset_refine_2d's
// text in flow2d_c_abi.h.  (A node's set-up and its record are written out in each kernel: shared, they moved registers in
// subset_refine2_kernel, whose instruction stream is kept as it is; profiles/subset_unified/README.md.)
#pragma once

#include <algorithm>

#include "node_grid.hpp"
#include "plane_sample.hpp"
#include "subset_sample.hpp"

constexpr int kSubsetMaxWaves = 4;
constexpr int kSubsetCounts = 7;                   // the counts of flow2d_subset_record that every entry writes
constexpr unsigned kSubsetLdsBytes = 64u * 1024u;  // what a launch may ask for without hipFuncSetAttribute
constexpr int kStateNoInput = -1, kStateFlat = -2, kStateStrayed = -3, kStateMasked = FLOW2D_SUBSET_STATE_MASKED;

// A wave's node: the frames of its instance, its four pixel arrays in LDS and its subset.  A kernel's own node derives from it.
struct SubsetNode {
    const float* f0;
    const float* f1;           // frame 1, or its B-spline coefficients
    double *fd, *fx, *fy, *g;  // the wave's LDS arrays
    int w, h, pitch;
    int cx, cy, R, side, n;
    int lane;
};

// The frame-0 window test: whether the subset of radius R about (cx, cy) lies inside the w x h frame.
__device__ __forceinline__ bool subset_inside_frame(int cx, int cy, int R, int w, int h)
{
    return cx - R >= 0 && cy - R >= 0 && cx + R <= w - 1 && cy + R <= h - 1;
}

// Frame 0 over the whole subset: f into the fd array, the central differences fx and fy, slot k pixel k's, filled by the lane that
// reads it afterwards.  Returns the lane's partial of the sum of f, in ascending k from 0.
template <typename Offset>
__device__ __forceinline__ double fill_frame_0(const SubsetNode& nd)
{
    const int left = nd.cx - nd.R, top = nd.cy - nd.R;
    double sum_f = 0.0;
    for (int k = nd.lane; k < nd.n; k += 64) {
        const int ky = k / nd.side, kx = k - ky * nd.side;
        const int x = left + kx, y = top + ky;
        const double f = sample_at<Offset>(nd.f0, x, y, nd.pitch);
        nd.fd[k] = f;
        nd.fx[k] = (sample_at<Offset>(nd.f0, min(x + 1, nd.w - 1), y, nd.pitch) - sample_at<Offset>(nd.f0, max(x - 1, 0), y, nd.pitch)) * 0.5;
        nd.fy[k] = (sample_at<Offset>(nd.f0, x, min(y + 1, nd.h - 1), nd.pitch) - sample_at<Offset>(nd.f0, x, max(y - 1, 0), nd.pitch)) * 0.5;
        sum_f += f;
    }
    return sum_f;
}

namespace flow2d {

// What a launch needs of the LDS: the doubles of one of a wave's four pixel arrays (N rounded up to a multiple of 2, at most 962),
// a wave's bytes and the waves of a workgroup -- four up to R = 10, three at 11 and 12, two beyond.
struct SubsetWaves {
    unsigned slice, wave_bytes, waves;
};

// Whether the planes of p's places lo .. hi in both halves of an array of n are all there (1), all absent (0) or given in part (-1).
template <typename Pointer>
int all_or_none(Pointer const* planes, int n, int lo, int hi)
{
    int there = 0, places = 0;
    for (int i = 0; i < n; ++i)
        if (i % (n / 2) >= lo && i % (n / 2) <= hi) {
            ++places;
            there += planes[i] != nullptr;
        }
    return there == 0 ? 0 : there == places ? 1 : -1;
}

// The host body of every subset refinement entry up to its launch, in the order of their refusals: the plane checks,
// subset_refine_args_status, the groups given all or none, the node planes, the node count, the alias check for one instance and,
// with the device entered, for the batch's span, and the records zeroed on the stream.  `start` and `out` hold n = 6 or 12 planes
// in the order of p (u, ux, uy[, uxx, uxy, uyy], v, ...; null = absent): the displacements are required, the gradients go all or
// none and so do the curvatures, and a start has curvatures only with gradients.  mask may be null.  extra_wave_bytes: what a wave
// keeps in LDS behind its four pixel arrays.
inline int subset_refine_enter(flow2d_context* ctx, const float* frame_0, const float* frame_1, const float* mask, size_t width,
                               size_t height, size_t pitch_bytes, const float* const* start, float* const* out, int n, float* out_score,
                               float* out_state, flow2d_subset_record* record, size_t nw, size_t nh, size_t node_pitch_bytes,
                               int grid_radius, int spacing, int min_radius, int subset_radius, int max_iterations, float epsilon,
                               std::initializer_list<float> bounds, unsigned extra_wave_bytes, SubsetWaves& lds)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    if (!planes_ok({frame_0, frame_1}, {mask}, width, height, pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    const int shared = subset_refine_args_status(width, height, nw, nh, grid_radius, spacing, min_radius, subset_radius, max_iterations,
                                                 epsilon, bounds, record);
    if (shared == FLOW2D_ERR_INVALID_ARGUMENT) return shared;
    const int started = all_or_none(start, n, 1, 2), curved = all_or_none(start, n, 3, 5);
    if (all_or_none(out, n, 1, 2) < 0 || all_or_none(out, n, 3, 5) < 0 || started < 0 || curved < 0 || (curved == 1 && started == 0))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; ++i)
        if (i % (n / 2) == 0 ? !planes_ok({start[i], out[i]}, {}, nw, nh, node_pitch_bytes)
                             : !planes_ok({}, {start[i], out[i]}, nw, nh, node_pitch_bytes))
            return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!planes_ok({}, {out_score, out_state}, nw, nh, node_pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (shared != FLOW2D_OK) return shared;  // (the node count)
    // the kernel reads frames, mask and nodes while other waves write: no written byte range may meet a read one or another written one
    auto aliased = [&](size_t frame_span, size_t node_span, size_t instances) {
        ByteRange written[15], read[15];
        for (int i = 0; i < 12; ++i) {
            written[i] = {i < n ? out[i] : nullptr, node_span};
            read[i] = {i < n ? start[i] : nullptr, node_span};
        }
        written[12] = {out_score, node_span};
        written[13] = {out_state, node_span};
        written[14] = {record, instances * sizeof(flow2d_subset_record)};
        read[12] = {frame_0, frame_span};
        read[13] = {frame_1, frame_span};
        read[14] = {mask, frame_span};
        return any_overlap(written, read);
    };
    if (aliased(height * pitch_bytes, nh * node_pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    if (aliased(batch_span(ctx, height * pitch_bytes), batch_span(ctx, nh * node_pitch_bytes), ctx->batch_count))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_HIP_TRY(clear_records(ctx, record));
    const unsigned side = static_cast<unsigned>(2 * subset_radius + 1);
    lds.slice = (side * side + 1u) & ~1u;
    lds.wave_bytes = 4u * lds.slice * sizeof(double) + extra_wave_bytes;  // at most 30 784 + extra
    lds.waves = std::min<unsigned>(kSubsetMaxWaves, kSubsetLdsBytes / lds.wave_bytes);
    return FLOW2D_OK;
}

}  // namespace flow2d

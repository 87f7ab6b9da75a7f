// The first level of a pyramid that starts from a prior flow, for gfx950: no reference counterpart (the reference's pyramid starts
// from zero at its coarsest level, optical_flow_2d.cpp:308-313).
//
// One launch does what flow2d_upsample_registration_2d does at every later level, with a full-resolution prior in place of the
// previous level's flow: the prior (u, v), made finite, is brought to the level's size by the area-weighted resample of
// flow2d_resample_xy_pair (x pass rounded to float, then y pass; here a DOWN-sample: an output sums in_w / w by in_h / h cells),
// stored as the level's base flow and handed in registers to the backward registration of the same pixel.  The normative
// definition is the one of flow2d_prior_registration_2d in flow2d_c_abi.h; the device functions are those of pyramid_ops.hip
// (pyramid_sample.hpp).  Built -ffp-contract=off: the bits follow that definition exactly.
//
// Memory-bound: per level pixel (in_w / w) * (in_h / h) prior pixels of two planes read once (neighbouring outputs share their
// border cells: cache hits), 12 bytes stored, 4 bytes of frame 0 or four gathers of frame 1 read.  Geometry of registration_kernel:
// 64 x 4 threads, four rows per thread one workgroup height apart, a wave's accesses of one row contiguous.
//
// The count of prior pixels that were not finite: the cells an output READS overlap its neighbours' (a cell cut by an output's
// border belongs to both), so each prior pixel is counted by the one output that OWNS it -- column g owns the prior columns
// [floor(g * delta_x), floor((g + 1) * delta_x)), the last one up to in_w, rows alike: the same float products the cells come
// from, monotone in g, so the ranges tile the prior exactly.  Counts are summed over the wave and added by one 64-bit integer
// atomic per wave that has any: the record does not depend on the order of the waves.
#include <cmath>

#include "plane_sample.hpp"
#include "pyramid_sample.hpp"

namespace {

constexpr int kPriorRows = 4;  // rows per thread: the geometry of registration_kernel

struct PriorArgs {
    const float *prior_u, *prior_v, *f0, *f1;
    float *out_u, *out_v, *warped;
    unsigned long long* record;  // one count per instance
    int w, h, in_w, in_h, pitch;
    ResampleXY k;
    float inv_hx, inv_hy;
};

template <typename Offset>
__global__ __launch_bounds__(flow2d::kPixelBlockX* flow2d::kPixelBlockY) void prior_registration_kernel(PriorArgs a, BatchArg batch)
{
    const size_t inst = batch_offset(batch);
    const float* __restrict__ prior_u = a.prior_u + inst;
    const float* __restrict__ prior_v = a.prior_v + inst;
    const float* __restrict__ f0 = a.f0 + inst;
    const float* __restrict__ f1 = a.f1 + inst;
    float* __restrict__ out_u = a.out_u + inst;
    float* __restrict__ out_v = a.out_v + inst;
    float* __restrict__ warped = a.warped + inst;
    const int gx = pixel_column();
    unsigned not_finite = 0;
    if (gx < a.w) {  // (no early return: every lane of the wave takes part in the sum of the counts below)
        const ResampleXCells c = resample_x_cells(gx, a.in_w, a.k);
        // the prior columns this output owns: up to the next output's first cell
        const int own_x_end = gx + 1 == a.w ? a.in_w : min(a.in_w, static_cast<int>(floorf(static_cast<float>(static_cast<unsigned>(gx) + 1u) * a.k.delta_x)));
        const int own_x = own_x_end - c.left_i;
        const int nx = max(c.cells_x, own_x);  // (left_i + nx <= in_w: both are cut at in_w)
#pragma unroll
        for (int r = 0; r < kPriorRows; ++r) {
            const int gy = static_cast<int>(pixel_row(kPriorRows, r));
            if (gy >= a.h) break;
            // the y cells of resample_2d.cu:77-118, as resample_xy_value (pyramid_ops.hip) forms them
            const float top_f = static_cast<float>(static_cast<unsigned>(gy)) * a.k.delta_y;
            const float bottom_f = static_cast<float>(static_cast<unsigned>(gy) + 1u) * a.k.delta_y;
            const int top_i = static_cast<int>(floorf(top_f));
            const int cells = min(a.in_h, static_cast<int>(ceilf(bottom_f))) - top_i;
            const int own_y_end = gy + 1 == a.h ? a.in_h : min(a.in_h, static_cast<int>(floorf(bottom_f)));
            const int own_y = own_y_end - top_i;
            const int ny = max(cells, own_y);
            float value_u = 0.f, value_v = 0.f;
            for (int j = 0; j < ny; ++j) {
                float frac = 1.f;
                if (j == 0) frac = static_cast<float>(top_i + 1) - top_f;
                if (j == cells - 1) frac = bottom_f - static_cast<float>(top_i + j);
                if (cells == 1) frac = a.k.delta_y;
                float x_pass_u = 0.f, x_pass_v = 0.f;  // the x pass of this prior row: first cell, whole cells, last cell (:56-72)
                for (int i = 0; i < nx; ++i) {
                    const Offset at = pixel_offset<Offset>(c.left_i + i, top_i + j, a.pitch);
                    float pu = load_at(prior_u, at), pv = load_at(prior_v, at);
                    const bool finite = fabsf(pu) < INFINITY && fabsf(pv) < INFINITY;  // (false for a NaN)
                    not_finite += (!finite && i < own_x && j < own_y) ? 1u : 0u;
                    pu = finite ? pu : 0.f;
                    pv = finite ? pv : 0.f;
                    if (i < c.cells_x) {
                        const float fx = i == 0 ? c.first_x : (i == c.cells_x - 1 ? c.last_x : 1.f);
                        x_pass_u += pu * fx;
                        x_pass_v += pv * fx;
                    }
                }
                if (j < cells) {
                    value_u += (x_pass_u * a.k.norm_x) * frac;
                    value_v += (x_pass_v * a.k.norm_x) * frac;
                }
            }
            const float uu = value_u * a.k.norm_y, vv = value_v * a.k.norm_y;
            const Offset o = pixel_offset<Offset>(gx, gy, a.pitch);
            store_at(out_u, o, uu);
            store_at(out_v, o, vv);
            const size_t at = static_cast<size_t>(gy) * a.pitch + gx;
            store_at(warped, o, registered_value(f0, f1, gx, gy, at, uu, vv, a.w, a.h, a.pitch, a.inv_hx, a.inv_hy));
        }
    }
    // a wave is one row of the workgroup (64 x 4): the sum of its lanes' counts, one atomic
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) not_finite += __shfl_xor(not_finite, step);
    if (threadIdx.x == 0 && not_finite) atomicAdd(a.record + blockIdx.z, static_cast<unsigned long long>(not_finite));
}

}  // namespace

extern "C" {

int flow2d_prior_registration_2d(flow2d_context* ctx, const float* prior_u, const float* prior_v, size_t in_width, size_t in_height,
                                 float* out_u, float* out_v, const float* frame_0, const float* frame_1, size_t width, size_t height,
                                 size_t pitch_bytes, float hx, float hy, float* output, unsigned long long* record)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    if (!flow2d::plane_args_ok(prior_u, in_width, in_height, pitch_bytes) || !flow2d::plane_args_ok(prior_v, in_width, in_height, pitch_bytes))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    const void* level_planes[] = {out_u, out_v, frame_0, frame_1, output};
    for (const void* p : level_planes)
        if (!flow2d::plane_args_ok(p, width, height, pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (width > in_width || height > in_height) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!record || (reinterpret_cast<uintptr_t>(record) % alignof(unsigned long long)) != 0) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!(std::isfinite(hx) && hx > 0.f) || !(std::isfinite(hy) && hy > 0.f)) return FLOW2D_ERR_INVALID_ARGUMENT;
    // the kernel marks every plane __restrict__: no written byte range may meet a read one or another written one
    const size_t prior_bytes = in_height * pitch_bytes, level_bytes = height * pitch_bytes;
    auto aliased = [&](size_t prior_span, size_t level_span, size_t instances) {
        const flow2d::ByteRange written[] = {{out_u, level_span}, {out_v, level_span}, {output, level_span},
                                             {record, instances * sizeof(unsigned long long)}};
        const flow2d::ByteRange read[] = {{prior_u, prior_span}, {prior_v, prior_span}, {frame_0, level_span}, {frame_1, level_span}};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(prior_bytes, level_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t instances = ctx->batch_count;
    if (aliased(flow2d::batch_span(ctx, prior_bytes), flow2d::batch_span(ctx, level_bytes), instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_HIP_TRY(hipMemsetAsync(record, 0, instances * sizeof(unsigned long long), ctx->stream));
    const PriorArgs a = {prior_u, prior_v, frame_0, frame_1, out_u, out_v, output, record,
                         static_cast<int>(width), static_cast<int>(height), static_cast<int>(in_width), static_cast<int>(in_height),
                         static_cast<int>(pitch_bytes / 4),
                         ResampleXY{static_cast<float>(in_width) / static_cast<float>(width), static_cast<float>(width) / static_cast<float>(in_width),
                                    static_cast<float>(in_height) / static_cast<float>(height), static_cast<float>(height) / static_cast<float>(in_height)},
                         1.f / hx, 1.f / hy};
    // (the largest offset a lane forms is into the prior, the tallest plane of the call: below in_height * pitch_bytes)
    flow2d::launch_by_span(prior_bytes, [&](auto offset) {
        prior_registration_kernel<decltype(offset)>
            <<<flow2d::pixel_grid(ctx, width, height, kPriorRows), flow2d::pixel_block(), 0, ctx->stream>>>(a, flow2d::batch_arg(ctx, 1));
    });
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"

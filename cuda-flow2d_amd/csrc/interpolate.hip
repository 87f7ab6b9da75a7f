// Occlusion-aware frame interpolation from a bidirectional flow for gfx950: no reference counterpart.
//
// output(x) = the frame at time t between frame_0 (t = 0) and frame_1 (t = 1): each side inverts its flow's linear trajectory
// by a K-step fixed point (where does the trajectory through x at time t start?), samples its frame there, and the two samples
// are blended with weights that prefer content both frames see.  The normative definition is the one of flow2d_interpolate_2d in
// flow2d_c_abi.h; the bilinear sample is the operation order of flow2d_consistency_2d (consistency.hip).  Built
// -ffp-contract=off and with the correctly rounded fp32 division: the bits follow that definition exactly.
//
// Geometry and sampler of plane_sample.hpp: 64 x 4 threads, four rows per thread.  Each side's fixed point is a chain of K + 1 dependent
// flow-pair gathers; the four rows and the two sides of a thread are eight independent chains, advanced step by step together
// so that a wave keeps eight gathers in flight instead of one.  One 32-bit byte offset per lane and chain serves the dwordx2
// column-pair gathers of both planes of a flow -- and, at the end, of the frame and the occlusion plane of that side -- against
// scalar plane bases.
#include <cmath>

#include "plane_sample.hpp"

namespace {

constexpr int kRows = 4;            // rows per thread
constexpr int kChains = 2 * kRows;  // chain r + kRows * side

// Where S(P, p) reads: p is replaced by the pixel itself when not finite, then clamped to the frame.
template <typename Offset>
__device__ __forceinline__ Tap<Offset> clamped_tap(float px, float py, float cx, float cy, int w, int h, int pitch)
{
    if (!(isfinite(px) && isfinite(py))) {
        px = cx;
        py = cy;
    }
    const float x_max = static_cast<float>(w - 1), y_max = static_cast<float>(h - 1);
    px = px < 0.f ? 0.f : (px > x_max ? x_max : px);
    py = py < 0.f ? 0.f : (py > y_max ? y_max : py);
    return make_tap<Offset>(px, py, w, h, pitch);
}

template <typename Offset>
__global__ __launch_bounds__(256) void interpolate_kernel(const float* __restrict__ frame_0, const float* __restrict__ frame_1,
                                                          const float* __restrict__ flow_u, const float* __restrict__ flow_v,
                                                          const float* __restrict__ back_u, const float* __restrict__ back_v,
                                                          const float* __restrict__ occ_0, const float* __restrict__ occ_1,
                                                          int w, int h, int pitch, float t, float s, int iterations,
                                                          float max_residual_sq, float* __restrict__ output, BatchArg batch)
{
    const size_t inst = batch_offset(batch);
    frame_0 += inst;
    frame_1 += inst;
    flow_u += inst;
    flow_v += inst;
    back_u += inst;
    back_v += inst;
    if (occ_0) occ_0 += inst;
    if (occ_1) occ_1 += inst;
    output += inst;
    const int gx = pixel_column();
    if (gx >= w) return;
    const float cx = static_cast<float>(gx);
    float cy[kRows];
#pragma unroll
    for (int i = 0; i < kRows; ++i)  // rows past the frame run on the last row and write nothing
        cy[i] = static_cast<float>(min(pixel_row(kRows, i), h - 1));

    // chain c: row c % kRows, side c / kRows (0: the forward flow and factor t, 1: the backward flow and factor s)
    float px[kChains], py[kChains], su[kChains], sv[kChains];
    Tap<Offset> tap[kChains];
#pragma unroll
    for (int c = 0; c < kChains; ++c) {
        px[c] = cx;
        py[c] = cy[c % kRows];
    }
    for (int k = 0; k <= iterations; ++k) {
        // step k samples the flow at p_k: p_{k+1} for k < K, the residual's sample for k = K
        float2 ga[kChains][2], gb[kChains][2];
#pragma unroll
        for (int c = 0; c < kChains; ++c) {
            tap[c] = clamped_tap<Offset>(px[c], py[c], cx, cy[c % kRows], w, h, pitch);
            const float* pu = c < kRows ? flow_u : back_u;
            const float* pv = c < kRows ? flow_v : back_v;
            ga[c][0] = column_pair(pu, tap[c].o0);
            gb[c][0] = column_pair(pu, tap[c].o1);
            ga[c][1] = column_pair(pv, tap[c].o0);
            gb[c][1] = column_pair(pv, tap[c].o1);
        }
#pragma unroll
        for (int c = 0; c < kChains; ++c) {
            su[c] = blend(tap[c], ga[c][0], gb[c][0]);
            sv[c] = blend(tap[c], ga[c][1], gb[c][1]);
        }
        if (k == iterations) break;
#pragma unroll
        for (int c = 0; c < kChains; ++c) {
            const float f = c < kRows ? t : s;
            px[c] = cx - f * su[c];
            py[c] = cy[c % kRows] - f * sv[c];
        }
    }
    // tap[c] is now the sample position of p_K / q_K; su / sv the flow sampled there
    float a[kChains], occ[kChains];
    bool ok[kChains];
#pragma unroll
    for (int c = 0; c < kChains; ++c) {
        const float* frame = c < kRows ? frame_0 : frame_1;
        a[c] = blend(tap[c], column_pair(frame, tap[c].o0), column_pair(frame, tap[c].o1));
        const float* mask = c < kRows ? occ_0 : occ_1;
        occ[c] = mask ? blend(tap[c], column_pair(mask, tap[c].o0), column_pair(mask, tap[c].o1)) : 0.f;
    }
    const float x_max = static_cast<float>(w - 1), y_max = static_cast<float>(h - 1);
#pragma unroll
    for (int c = 0; c < kChains; ++c) {
        const float f = c < kRows ? t : s;
        const float rx = cx - f * su[c] - px[c];
        const float ry = cy[c % kRows] - f * sv[c] - py[c];
        // a non-finite p_K fails the range test
        ok[c] = px[c] >= 0.f && px[c] <= x_max && py[c] >= 0.f && py[c] <= y_max && rx * rx + ry * ry <= max_residual_sq;
        float o = ok[c] ? occ[c] : 0.f;
        if (!(o <= 1.f)) o = 1.f;  // NaN: occluded
        if (!(o >= 0.f)) o = 0.f;
        occ[c] = o;
    }
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
        const int gy = pixel_row(kRows, i);
        if (gy >= h) return;
        const float ok0 = ok[i] ? 1.f : 0.f, ok1 = ok[i + kRows] ? 1.f : 0.f;
        const float a0 = a[i], a1 = a[i + kRows];
        const float v0 = ok0 * (1.f - occ[i]), v1 = ok1 * (1.f - occ[i + kRows]);
        float w0, w1;
        if (v0 + v1 > 0.f) {  // seen in both frames wins over seen in one
            w0 = s * v0;
            w1 = t * v1;
        } else {
            w0 = s * ok0;
            w1 = t * ok1;
        }
        const float out = (w0 + w1 > 0.f) ? (w0 * a0 + w1 * a1) / (w0 + w1) : s * a0 + t * a1;
        output[static_cast<Offset>(gy) * static_cast<Offset>(pitch) + static_cast<Offset>(gx)] = out;
    }
}

}  // namespace

extern "C" {

int flow2d_interpolate_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1, const float* flow_u, const float* flow_v,
                          const float* back_u, const float* back_v, const float* occlusion_0, const float* occlusion_1,
                          size_t width, size_t height, size_t pitch_bytes, float t, int iterations, float max_residual,
                          float* output)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    const float* inputs[] = {frame_0, frame_1, flow_u, flow_v, back_u, back_v, occlusion_0, occlusion_1};
    for (int i = 0; i < 8; ++i)
        if ((i < 6 || inputs[i] != nullptr) && !flow2d::plane_args_ok(inputs[i], width, height, pitch_bytes))
            return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::plane_args_ok(output, width, height, pitch_bytes) || !std::isfinite(t) || t < 0.f || t > 1.f ||
        iterations < 1 || iterations > 16 || !std::isfinite(max_residual) || max_residual < 0.f)
        return FLOW2D_ERR_INVALID_ARGUMENT;
    // the kernel marks every plane __restrict__: the written byte range must not meet any read one
    auto aliased = [&](size_t span) {
        const flow2d::ByteRange written[] = {{output, span}};
        flow2d::ByteRange read[8];
        for (int i = 0; i < 8; ++i) read[i] = {inputs[i], span};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(height * pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    if (aliased(flow2d::batch_span(ctx, height * pitch_bytes))) return FLOW2D_ERR_INVALID_ARGUMENT;
    const float s = 1.f - t;
    const float max_residual_sq = max_residual * max_residual;
    flow2d::launch_by_span(height * pitch_bytes, [&](auto offset) {
        interpolate_kernel<decltype(offset)><<<flow2d::pixel_grid(ctx, width, height, kRows), flow2d::pixel_block(), 0, ctx->stream>>>(
            frame_0, frame_1, flow_u, flow_v, back_u, back_v, occlusion_0, occlusion_1, (int)width, (int)height,
            (int)(pitch_bytes / 4), t, s, iterations, max_residual_sq, output, flow2d::batch_arg(ctx, 1));
    });
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"

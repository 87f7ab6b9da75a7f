// Motion-compensated temporal denoising for gfx950: no reference counterpart.
//
// flow2d_denoise_2d: output(x) = the weighted mean of the centre frame at x and of N neighbour frames sampled where the flow
// from the centre to each of them points, without what the occlusion masks mark and, with range_sigma > 0, with a rational
// photometric weight.  flow2d_compose_flow_2d: the flow a -> c on a's grid from a -> b and b -> c, which is how neighbours
// further than one frame away are reached.  The normative definitions are those of the two entries in flow2d_c_abi.h; the
// bilinear sample is the operation order of flow2d_consistency_2d (consistency.hip).  Built -ffp-contract=off and with the
// correctly rounded fp32 division: the bits follow those definitions exactly.
//
// Geometry and sampler of plane_sample.hpp: 64 x 4 threads, kRows rows per thread, one byte offset per lane (32 bits when the
// plane's span allows) against scalar plane bases, column-pair dwordx2 gathers.  There is no dependent gather chain: the coalesced loads
// (flow, mask) of all neighbours and rows of a thread are issued first, then all gathers, then the sums in neighbour order.
// The kernel is templated on N so that the loops unroll and the pointer table stays in scalar registers; rows per thread fall
// with N (rows x N <= 8) so that the loads in flight fit the register file without scratch.
// Per pixel 8 + 16 N algorithmic bytes (12 N without masks): memory-bound.
#include <cmath>

#include "plane_sample.hpp"

namespace {

constexpr int kComposeRows = 4;  // rows per thread
constexpr int kMaxNeighbours = FLOW2D_DENOISE_MAX_NEIGHBOURS;
constexpr unsigned kQuietNaN = 0x7fc00000u;

constexpr int denoise_rows(int n) { return n <= 2 ? 4 : (n <= 4 ? 2 : 1); }

template <int N>
struct DenoiseNeighbours {
    const float* frame[N];
    const float* flow_u[N];
    const float* flow_v[N];
    const float* occlusion[N];  // entries may be null
};

template <int N, typename Offset>
__global__ __launch_bounds__(256) void denoise_kernel(const float* __restrict__ centre, DenoiseNeighbours<N> nb, int w, int h,
                                                      int pitch, float range_sigma, float* __restrict__ output,
                                                      float* __restrict__ weight_sum, BatchArg batch)
{
    constexpr int R = denoise_rows(N);
    const size_t inst = batch_offset(batch);
    centre += inst;
    output += inst;
    if (weight_sum) weight_sum += inst;
    const int gx = pixel_column();
    if (gx >= w) return;
    const float cx = static_cast<float>(gx);
    const float x_max = static_cast<float>(w - 1), y_max = static_cast<float>(h - 1);

    // the coalesced loads of every row and neighbour (rows past the frame run on the last row and write nothing)
    float cy[R], c[R], fu[R][N], fv[R][N], m[R][N];
    Offset at[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int gy = min(pixel_row(R, i), h - 1);
        cy[i] = static_cast<float>(gy);
        at[i] = pixel_offset<Offset>(gx, gy, pitch);
        c[i] = load_at(centre, at[i]);
#pragma unroll
        for (int n = 0; n < N; ++n) {
            fu[i][n] = load_at(nb.flow_u[n] + inst, at[i]);
            fv[i][n] = load_at(nb.flow_v[n] + inst, at[i]);
            m[i][n] = nb.occlusion[n] ? load_at(nb.occlusion[n] + inst, at[i]) : 0.f;
        }
    }
    // every gather
    Tap<Offset> tap[R][N];
    float2 ga[R][N], gb[R][N];
    bool ok[R][N];
#pragma unroll
    for (int i = 0; i < R; ++i) {
#pragma unroll
        for (int n = 0; n < N; ++n) {
            float qx = cx + fu[i][n], qy = cy[i] + fv[i][n];
            ok[i][n] = qx >= 0.f && qx <= x_max && qy >= 0.f && qy <= y_max;  // a NaN or an infinity fails
            if (!ok[i][n]) {
                qx = cx;
                qy = cy[i];
            }
            tap[i][n] = make_tap<Offset>(qx, qy, w, h, pitch);
            ga[i][n] = column_pair(nb.frame[n] + inst, tap[i][n].o0);
            gb[i][n] = column_pair(nb.frame[n] + inst, tap[i][n].o1);
        }
    }
    // the sums, in neighbour order
    const float sigma_sq = range_sigma * range_sigma;
    float out[R], den_out[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        float num = c[i], den = 1.f;
#pragma unroll
        for (int n = 0; n < N; ++n) {
            const float s = blend(tap[i][n], ga[i][n], gb[i][n]);
            float mm = m[i][n];
            if (!(mm <= 1.f)) mm = 1.f;  // NaN: occluded
            if (!(mm >= 0.f)) mm = 0.f;
            const float d = s - c[i];
            const float g = range_sigma == 0.f ? 1.f : sigma_sq / (sigma_sq + d * d);
            float wgt = ok[i][n] ? (1.f - mm) * g : 0.f;
            float t = wgt * s;
            if (!isfinite(t)) {  // a NaN or infinite sample, a NaN weight
                wgt = 0.f;
                t = 0.f;
            }
            num = num + t;
            den = den + wgt;
        }
        out[i] = num / den;
        den_out[i] = den;
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int gy = pixel_row(R, i);
        if (gy >= h) return;
        store_at(output, at[i], out[i]);
        if (weight_sum) store_at(weight_sum, at[i], den_out[i]);
    }
}

__device__ __forceinline__ float canonical_nan(float r)
{
    const unsigned bits = __float_as_uint(r);
    return (bits & 0x7fffffffu) > 0x7f800000u ? __uint_as_float(kQuietNaN) : r;
}

template <typename Offset>
__global__ __launch_bounds__(256) void compose_kernel(const float* __restrict__ ab_u, const float* __restrict__ ab_v,
                                                      const float* __restrict__ bc_u, const float* __restrict__ bc_v,
                                                      const float* __restrict__ mask_ab, const float* __restrict__ mask_bc,
                                                      int w, int h, int pitch, float* __restrict__ out_u,
                                                      float* __restrict__ out_v, float* __restrict__ out_mask, BatchArg batch)
{
    const size_t inst = batch_offset(batch);
    ab_u += inst;
    ab_v += inst;
    bc_u += inst;
    bc_v += inst;
    if (mask_ab) mask_ab += inst;
    if (mask_bc) mask_bc += inst;
    out_u += inst;
    out_v += inst;
    if (out_mask) out_mask += inst;
    const int gx = pixel_column();
    if (gx >= w) return;
    const float cx = static_cast<float>(gx);
    const float x_max = static_cast<float>(w - 1), y_max = static_cast<float>(h - 1);
    const bool masks = out_mask != nullptr;

    float cy[kComposeRows], fu[kComposeRows], fv[kComposeRows], ma[kComposeRows];
    Offset at[kComposeRows];
#pragma unroll
    for (int i = 0; i < kComposeRows; ++i) {
        const int gy = min(pixel_row(kComposeRows, i), h - 1);
        cy[i] = static_cast<float>(gy);
        at[i] = pixel_offset<Offset>(gx, gy, pitch);
        fu[i] = load_at(ab_u, at[i]);
        fv[i] = load_at(ab_v, at[i]);
        ma[i] = (masks && mask_ab) ? load_at(mask_ab, at[i]) : 0.f;
    }
    Tap<Offset> tap[kComposeRows];
    float2 ga[kComposeRows][3], gb[kComposeRows][3];
    bool ok[kComposeRows];
#pragma unroll
    for (int i = 0; i < kComposeRows; ++i) {
        float qx = cx + fu[i], qy = cy[i] + fv[i];
        ok[i] = qx >= 0.f && qx <= x_max && qy >= 0.f && qy <= y_max;  // a NaN or an infinity fails
        if (!ok[i]) {  // sampled at the pixel itself and not used
            qx = cx;
            qy = cy[i];
        }
        tap[i] = make_tap<Offset>(qx, qy, w, h, pitch);
        ga[i][0] = column_pair(bc_u, tap[i].o0);
        gb[i][0] = column_pair(bc_u, tap[i].o1);
        ga[i][1] = column_pair(bc_v, tap[i].o0);
        gb[i][1] = column_pair(bc_v, tap[i].o1);
        if (masks && mask_bc) {
            ga[i][2] = column_pair(mask_bc, tap[i].o0);
            gb[i][2] = column_pair(mask_bc, tap[i].o1);
        } else {
            ga[i][2] = gb[i][2] = make_float2(0.f, 0.f);
        }
    }
#pragma unroll
    for (int i = 0; i < kComposeRows; ++i) {
        const int gy = pixel_row(kComposeRows, i);
        if (gy >= h) return;
        const float nan = __uint_as_float(kQuietNaN);
        const float su = blend(tap[i], ga[i][0], gb[i][0]);
        const float sv = blend(tap[i], ga[i][1], gb[i][1]);
        store_at(out_u, at[i], ok[i] ? canonical_nan(fu[i] + su) : nan);
        store_at(out_v, at[i], ok[i] ? canonical_nan(fv[i] + sv) : nan);
        if (masks) {
            const float sm = blend(tap[i], ga[i][2], gb[i][2]);
            store_at(out_mask, at[i], (!ok[i] || !(ma[i] == 0.f) || !(sm <= 0.f)) ? 1.f : 0.f);
        }
    }
}

template <int N>
void launch_denoise(flow2d_context* ctx, const float* centre, const float* const* frames, const float* const* flows_u,
                    const float* const* flows_v, const float* const* occlusions, size_t width, size_t height,
                    size_t pitch_bytes, float range_sigma, float* output, float* weight_sum)
{
    DenoiseNeighbours<N> nb;
    for (int n = 0; n < N; ++n) {
        nb.frame[n] = frames[n];
        nb.flow_u[n] = flows_u[n];
        nb.flow_v[n] = flows_v[n];
        nb.occlusion[n] = occlusions ? occlusions[n] : nullptr;
    }
    flow2d::launch_by_span(height * pitch_bytes, [&](auto offset) {
        denoise_kernel<N, decltype(offset)><<<flow2d::pixel_grid(ctx, width, height, denoise_rows(N)), flow2d::pixel_block(), 0,
                                              ctx->stream>>>(centre, nb, (int)width, (int)height, (int)(pitch_bytes / 4), range_sigma,
                                                             output, weight_sum, flow2d::batch_arg(ctx, 1));
    });
}

}  // namespace

extern "C" {

int flow2d_denoise_2d(flow2d_context* ctx, const float* centre, size_t neighbour_count, const float* const* frames,
                      const float* const* flows_u, const float* const* flows_v, const float* const* occlusions, size_t width,
                      size_t height, size_t pitch_bytes, float range_sigma, float* output, float* weight_sum)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    if (neighbour_count < 1 || neighbour_count > kMaxNeighbours || !frames || !flows_u || !flows_v) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(range_sigma) || range_sigma < 0.f) return FLOW2D_ERR_INVALID_ARGUMENT;
    const float* inputs[1 + 4 * kMaxNeighbours];
    size_t input_count = 0;
    inputs[input_count++] = centre;
    for (size_t n = 0; n < neighbour_count; ++n) {
        inputs[input_count++] = frames[n];
        inputs[input_count++] = flows_u[n];
        inputs[input_count++] = flows_v[n];
        if (occlusions && occlusions[n]) inputs[input_count++] = occlusions[n];
    }
    for (size_t k = 0; k < input_count; ++k)
        if (!flow2d::plane_args_ok(inputs[k], width, height, pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::plane_args_ok(output, width, height, pitch_bytes) ||
        (weight_sum && !flow2d::plane_args_ok(weight_sum, width, height, pitch_bytes)))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    // the written byte ranges must not meet any read one (not only its base), nor each other
    auto aliased = [&](size_t span) {
        const flow2d::ByteRange written[] = {{output, span}, {weight_sum, span}};
        flow2d::ByteRange read[1 + 4 * kMaxNeighbours];
        for (size_t k = 0; k < input_count; ++k) read[k] = {inputs[k], span};
        return flow2d::any_overlap(written, 2, read, input_count);
    };
    if (aliased(height * pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    if (aliased(flow2d::batch_span(ctx, height * pitch_bytes))) return FLOW2D_ERR_INVALID_ARGUMENT;
#define FLOW2D_DENOISE_CASE(N)                                                                                              \
    case N:                                                                                                                 \
        launch_denoise<N>(ctx, centre, frames, flows_u, flows_v, occlusions, width, height, pitch_bytes, range_sigma, output, \
                          weight_sum);                                                                                      \
        break
    switch (neighbour_count) {
        FLOW2D_DENOISE_CASE(1);
        FLOW2D_DENOISE_CASE(2);
        FLOW2D_DENOISE_CASE(3);
        FLOW2D_DENOISE_CASE(4);
        FLOW2D_DENOISE_CASE(5);
        FLOW2D_DENOISE_CASE(6);
        FLOW2D_DENOISE_CASE(7);
        FLOW2D_DENOISE_CASE(8);
    }
#undef FLOW2D_DENOISE_CASE
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

int flow2d_compose_flow_2d(flow2d_context* ctx, const float* ab_u, const float* ab_v, const float* bc_u, const float* bc_v,
                           const float* mask_ab, const float* mask_bc, size_t width, size_t height, size_t pitch_bytes,
                           float* out_u, float* out_v, float* out_mask)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    const float* inputs[] = {ab_u, ab_v, bc_u, bc_v, mask_ab, mask_bc};
    float* const written[] = {out_u, out_v, out_mask};
    for (int i = 0; i < 6; ++i)
        if ((i < 4 || inputs[i] != nullptr) && !flow2d::plane_args_ok(inputs[i], width, height, pitch_bytes))
            return FLOW2D_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < 3; ++i)
        if ((i < 2 || written[i] != nullptr) && !flow2d::plane_args_ok(written[i], width, height, pitch_bytes))
            return FLOW2D_ERR_INVALID_ARGUMENT;
    // the written byte ranges must not meet any read one (not only its base), nor each other
    auto aliased = [&](size_t span) {
        flow2d::ByteRange out[3], in[6];
        for (int i = 0; i < 3; ++i) out[i] = {written[i], span};
        for (int i = 0; i < 6; ++i) in[i] = {inputs[i], span};
        return flow2d::any_overlap(out, in);
    };
    if (aliased(height * pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    if (aliased(flow2d::batch_span(ctx, height * pitch_bytes))) return FLOW2D_ERR_INVALID_ARGUMENT;
    flow2d::launch_by_span(height * pitch_bytes, [&](auto offset) {
        compose_kernel<decltype(offset)><<<flow2d::pixel_grid(ctx, width, height, kComposeRows), flow2d::pixel_block(), 0, ctx->stream>>>(
            ab_u, ab_v, bc_u, bc_v, mask_ab, mask_bc, (int)width, (int)height, (int)(pitch_bytes / 4), out_u, out_v, out_mask,
            flow2d::batch_arg(ctx, 1));
    });
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"

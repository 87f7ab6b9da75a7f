// Occlusion-aware frame interpolation from a bidirectional flow for gfx950: no reference counterpart.
//
// output(x) = the frame at time t between frame_0 (t = 0) and frame_1 (t = 1): each side inverts its flow's linear trajectory
// by a K-step fixed point (where does the trajectory through x at time t start?), samples its frame there, and the two samples
// are blended with weights that prefer content both frames see.  The normative definition is the one of flow2d_interpolate_2d in
// flow2d_c_abi.h; the bilinear sample is the operation order of flow2d_consistency_2d (consistency.hip).  Built
// -ffp-contract=off and with the correctly rounded fp32 division: the bits follow that definition exactly.
//
// Geometry of consistency.hip: 64 x 4 threads, four rows per thread.  Each side's fixed point is a chain of K + 1 dependent
// flow-pair gathers; the four rows and the two sides of a thread are eight independent chains, advanced step by step together
// so that a wave keeps eight gathers in flight instead of one.  One 32-bit byte offset per lane and chain serves the dwordx2
// column-pair gathers of both planes of a flow -- and, at the end, of the frame and the occlusion plane of that side -- against
// scalar plane bases.
#include <cmath>

#include "common.hpp"

namespace {

constexpr int kBlockX = 64;
constexpr int kBlockY = 4;
constexpr int kRows = 4;     // rows per thread: the geometry of consistency_kernel
constexpr int kChains = 2 * kRows;  // chain r + kRows * side

template <typename Offset>
__device__ __forceinline__ float2 column_pair(const float* __restrict__ base, Offset byte_offset)
{
    const float* p = reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_offset);
    return make_float2(p[0], p[1]);
}

// Where S(P, p) reads and with which weights: p is replaced by the pixel itself when not finite, then clamped to the frame.
template <typename Offset>
struct Tap {
    Offset o0, o1;       // byte offsets of the column pairs (xb, xb + 1) in rows y and y1
    float w00, w01, w10, w11;
    bool x_second, x1_second;
};

template <typename Offset>
__device__ __forceinline__ Tap<Offset> make_tap(float px, float py, float cx, float cy, int w, int h, int pitch)
{
    if (!(isfinite(px) && isfinite(py))) {
        px = cx;
        py = cy;
    }
    const float x_max = static_cast<float>(w - 1), y_max = static_cast<float>(h - 1);
    px = px < 0.f ? 0.f : (px > x_max ? x_max : px);
    py = py < 0.f ? 0.f : (py > y_max ? y_max : py);
    const int x = static_cast<int>(floorf(px));
    const int y = static_cast<int>(floorf(py));
    const float dx = px - static_cast<float>(x);
    const float dy = py - static_cast<float>(y);
    const int x1 = min(w - 1, x + 1);
    const int y1 = min(h - 1, y + 1);
    // the column pair (xb, xb + 1), xb = min(x, w - 2), holds x and x1 (w = 1: the second column is row padding, never selected)
    const int xb = max(min(x, w - 2), 0);
    Tap<Offset> t;
    t.o0 = (static_cast<Offset>(y) * static_cast<Offset>(pitch) + static_cast<Offset>(xb)) * sizeof(float);
    t.o1 = (static_cast<Offset>(y1) * static_cast<Offset>(pitch) + static_cast<Offset>(xb)) * sizeof(float);
    t.w00 = (1.f - dx) * (1.f - dy);
    t.w01 = (dx) * (1.f - dy);
    t.w10 = (1.f - dx) * (dy);
    t.w11 = (dx) * (dy);
    t.x_second = x != xb;
    t.x1_second = x1 != xb;
    return t;
}

template <typename Offset>
__device__ __forceinline__ float blend(const Tap<Offset>& t, float2 a, float2 b)
{
    return t.w00 * (t.x_second ? a.y : a.x) + t.w01 * (t.x1_second ? a.y : a.x) + t.w10 * (t.x_second ? b.y : b.x) +
           t.w11 * (t.x1_second ? b.y : b.x);
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
    const int gx = blockIdx.x * kBlockX + threadIdx.x;
    if (gx >= w) return;
    const float cx = static_cast<float>(gx);
    float cy[kRows];
#pragma unroll
    for (int i = 0; i < kRows; ++i)  // rows past the frame run on the last row and write nothing
        cy[i] = static_cast<float>(min((blockIdx.y * kRows + i) * kBlockY + threadIdx.y, h - 1));

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
            tap[c] = make_tap<Offset>(px[c], py[c], cx, cy[c % kRows], w, h, pitch);
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
        const int gy = (blockIdx.y * kRows + i) * kBlockY + threadIdx.y;
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

inline bool ranges_overlap(const void* a, const void* b, size_t bytes)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + bytes && pb < pa + bytes;
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
    // the kernel marks every plane __restrict__: the written byte range must not meet any read one (not only its base)
    for (const float* p : inputs)
        if (p && ranges_overlap(output, p, height * pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    // a lock-step batch: instance b of every plane at + b * stride, so each plane spans all instances
    const size_t span = height * pitch_bytes + (ctx->batch_count - 1) * ctx->batch_stride_floats * sizeof(float);
    for (const float* p : inputs)
        if (p && ranges_overlap(output, p, span)) return FLOW2D_ERR_INVALID_ARGUMENT;
    const float s = 1.f - t;
    const float max_residual_sq = max_residual * max_residual;
    dim3 grid(flow2d::div_up(width, kBlockX), flow2d::div_up(flow2d::div_up(height, kRows), kBlockY), flow2d::batch_z(ctx, 1));
    const BatchArg batch = flow2d::batch_arg(ctx, 1);
    // 32-bit per-lane offsets when the largest one a lane forms -- (height - 1) * pitch + width + 1 floats, in bytes -- fits
    if (height * pitch_bytes < (size_t(1) << 32))
        interpolate_kernel<unsigned><<<grid, dim3(kBlockX, kBlockY), 0, ctx->stream>>>(
            frame_0, frame_1, flow_u, flow_v, back_u, back_v, occlusion_0, occlusion_1, (int)width, (int)height,
            (int)(pitch_bytes / 4), t, s, iterations, max_residual_sq, output, batch);
    else
        interpolate_kernel<size_t><<<grid, dim3(kBlockX, kBlockY), 0, ctx->stream>>>(
            frame_0, frame_1, flow_u, flow_v, back_u, back_v, occlusion_0, occlusion_1, (int)width, (int)height,
            (int)(pitch_bytes / 4), t, s, iterations, max_residual_sq, output, batch);
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"

// Error statistics of a flow estimate against ground truth for gfx950: no reference counterpart.
//
// Per pixel the endpoint error, the angular error and the class of flow2d_flow_error_2d (normative definition in
// flow2d_c_abi.h), summed into one record per lock-step instance.  Built -ffp-contract=off: the EPE plane follows that
// definition bit for bit.
//
// Memory-bound: 16 bytes of flow and ground truth per pixel (20 with an occlusion plane), read as dwordx4 per lane -- a wave
// covers 256 columns of one row --, and 4 bytes per per-pixel plane written.  Two launches, no atomics: every workgroup
// reduces its 256 x 32 pixels in a fixed order (rows, then the four columns of a lane, then the reduction of
// ordered_reduce.hpp) into a slab of the workspace, and one workgroup per instance sums the slabs in block order.  The grid,
// and with it the order of every double addition, depends only on (width, height): repeated calls and batch instances give
// the same bytes.
#include <cfloat>
#include <cmath>

#include "ordered_reduce.hpp"
#include "plane_sample.hpp"

namespace {

constexpr int kLanesX = 64;         // lanes of a wave along x, four columns each
constexpr int kWavesY = 4;          // waves of a workgroup, one row apart
constexpr int kRowsPerThread = 8;
constexpr int kBlockCols = kLanesX * 4;                 // 256
constexpr int kBlockRows = kWavesY * kRowsPerThread;    // 32
constexpr int kFinalThreads = 256;
constexpr float kDegrees = 57.29577951308232f;

// Sums over pixels, classes noc (0) and occ (1); all = noc + occ is formed by the final kernel.  Count: unsigned in a
// per-workgroup slab (FlowErrorPartial), 64 bits in the final kernel.
template <typename Count>
struct FlowErrorSums {
    double sum[2][3];     // epe, epe^2, ae
    float max_epe[2];
    Count count[2][6];    // count, above 0.5 / 1 / 2 / 3, fl
    Count invalid, nonfinite;

    template <typename Other>
    __device__ __forceinline__ void combine(const Other& q)
    {
        for (int k = 0; k < 2; ++k) {
            for (int j = 0; j < 3; ++j) sum[k][j] += q.sum[k][j];
            max_epe[k] = fmaxf(max_epe[k], q.max_epe[k]);
            for (int j = 0; j < 6; ++j) count[k][j] += q.count[k][j];
        }
        invalid += q.invalid;
        nonfinite += q.nonfinite;
    }
    __device__ __forceinline__ void across_lanes()
    {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
#pragma unroll
            for (int j = 0; j < 3; ++j) sum[k][j] = wave_sum(sum[k][j]);
            max_epe[k] = wave_max(max_epe[k]);
#pragma unroll
            for (int j = 0; j < 6; ++j) count[k][j] = wave_sum(count[k][j]);
        }
        invalid = wave_sum(invalid);
        nonfinite = wave_sum(nonfinite);
    }
};
using FlowErrorPartial = FlowErrorSums<unsigned>;
static_assert(sizeof(FlowErrorPartial) % 16 == 0, "slabs stay 16-byte aligned");

struct ClassAcc {
    double s_epe = 0.0, s_epe_sq = 0.0, s_ae = 0.0;
    float max_epe = 0.f;
    unsigned n = 0, a05 = 0, a1 = 0, a2 = 0, a3 = 0, fl = 0;

    // predicated, not branched: a class picked per pixel through a pointer or an index ends in scratch.  Adding +0.0 leaves
    // every sum's bits as they are (the sums start at +0 and every term is >= 0, inf or NaN).
    __device__ __forceinline__ void add_if(bool take, float epe, float ae, float gmag)
    {
        const double e = take ? static_cast<double>(epe) : 0.0;
        s_epe += e;
        s_epe_sq += e * e;
        s_ae += take ? static_cast<double>(ae) : 0.0;
        max_epe = take ? fmaxf(max_epe, epe) : max_epe;
        n += take;
        a05 += take & (epe > 0.5f);
        a1 += take & (epe > 1.f);
        a2 += take & (epe > 2.f);
        a3 += take & (epe > 3.f);
        fl += take & (epe > 3.f) & (epe > 0.05f * gmag);
    }
};

struct Acc {
    ClassAcc noc, occ;
    unsigned invalid = 0, nonfinite = 0;
};

// One pixel of the definition: accumulates it and returns its (epe, ae), NaN where it takes no part.
__device__ __forceinline__ void error_pixel(float u, float v, float gu, float gv, bool occluded, Acc& acc, float& epe_out,
                                            float& ae_out)
{
    epe_out = ae_out = __builtin_nanf("");
    if (!(fabsf(gu) <= 1e9f && fabsf(gv) <= 1e9f)) {  // NaN and inf fail the comparison
        ++acc.invalid;
        return;
    }
    if (!(fabsf(u) <= FLT_MAX && fabsf(v) <= FLT_MAX)) {
        ++acc.nonfinite;
        return;
    }
    const float du = u - gu, dv = v - gv;
    const float epe = sqrtf(du * du + dv * dv);
    const float cx = v - gv, cy = gu - u, cz = u * gv - v * gu;
    const float cross = sqrtf((cx * cx + cy * cy) + cz * cz);
    const float dot = (u * gu + v * gv) + 1.f;
    const float ae = atan2f(cross, dot) * kDegrees;
    const float gmag = sqrtf(gu * gu + gv * gv);
    acc.noc.add_if(!occluded, epe, ae, gmag);
    acc.occ.add_if(occluded, epe, ae, gmag);
    epe_out = epe;
    ae_out = ae;
}

// Offset: unsigned (a plane's whole extent fits 32 bits) or size_t; HasMask: an occlusion plane is read.
template <typename Offset, bool HasMask>
__global__ __launch_bounds__(256) void flow_error_partials_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                                  const float* __restrict__ gt_u, const float* __restrict__ gt_v,
                                                                  const float* __restrict__ occlusion, int w, int h, int pitch,
                                                                  float* __restrict__ epe, float* __restrict__ ae,
                                                                  FlowErrorPartial* __restrict__ partials, BatchArg batch)
{
    const size_t inst = batch_offset(batch);
    u += inst;
    v += inst;
    gt_u += inst;
    gt_v += inst;
    if (HasMask) occlusion += inst;
    if (epe) epe += inst;
    if (ae) ae += inst;
    const int x0 = (blockIdx.x * kLanesX + threadIdx.x) * 4;
    Acc acc;
    if (x0 < w) {
#pragma unroll 2
        for (int i = 0; i < kRowsPerThread; ++i) {
            const int gy = blockIdx.y * kBlockRows + i * kWavesY + threadIdx.y;
            if (gy >= h) break;
            // x0 < w and the pitch is a multiple of four floats: the four columns lie inside the row, padding included
            const Offset c = static_cast<Offset>(gy) * static_cast<Offset>(pitch) + static_cast<Offset>(x0);
            const float4 fu = *reinterpret_cast<const float4*>(u + c);
            const float4 fv = *reinterpret_cast<const float4*>(v + c);
            const float4 tu = *reinterpret_cast<const float4*>(gt_u + c);
            const float4 tv = *reinterpret_cast<const float4*>(gt_v + c);
            float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
            if (HasMask) m = *reinterpret_cast<const float4*>(occlusion + c);
            const int n = min(4, w - x0);
            float4 e, a;
            error_pixel(fu.x, fv.x, tu.x, tv.x, m.x != 0.f, acc, e.x, a.x);
            if (n > 1) error_pixel(fu.y, fv.y, tu.y, tv.y, m.y != 0.f, acc, e.y, a.y);
            if (n > 2) error_pixel(fu.z, fv.z, tu.z, tv.z, m.z != 0.f, acc, e.z, a.z);
            if (n > 3) error_pixel(fu.w, fv.w, tu.w, tv.w, m.w != 0.f, acc, e.w, a.w);
            // the columns beyond the width belong to the caller (a level in a larger container): never written
            if (n == 4) {
                if (epe) *reinterpret_cast<float4*>(epe + c) = e;
                if (ae) *reinterpret_cast<float4*>(ae + c) = a;
            } else {
                if (epe) {
                    epe[c] = e.x;
                    if (n > 1) epe[c + 1] = e.y;
                    if (n > 2) epe[c + 2] = e.z;
                }
                if (ae) {
                    ae[c] = a.x;
                    if (n > 1) ae[c + 1] = a.y;
                    if (n > 2) ae[c + 2] = a.z;
                }
            }
        }
    }
    FlowErrorPartial mine;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const ClassAcc& c = k ? acc.occ : acc.noc;
        mine.sum[k][0] = c.s_epe;
        mine.sum[k][1] = c.s_epe_sq;
        mine.sum[k][2] = c.s_ae;
        mine.max_epe[k] = c.max_epe;
        const unsigned counts[6] = {c.n, c.a05, c.a1, c.a2, c.a3, c.fl};
#pragma unroll
        for (int j = 0; j < 6; ++j) mine.count[k][j] = counts[j];
    }
    mine.invalid = acc.invalid;
    mine.nonfinite = acc.nonfinite;
    if (workgroup_reduce<kWavesY>(mine, threadIdx.x, threadIdx.y))
        partials[static_cast<size_t>(blockIdx.z) * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] = mine;
}

// One workgroup per instance: thread t sums slabs t, t + 256, ... in order, then the reduction of ordered_reduce.hpp.
__global__ __launch_bounds__(kFinalThreads) void flow_error_final_kernel(const FlowErrorPartial* __restrict__ partials,
                                                                         unsigned blocks, flow2d_flow_error_stats* __restrict__ stats)
{
    const FlowErrorPartial* slab = partials + static_cast<size_t>(blockIdx.x) * blocks;
    FlowErrorSums<unsigned long long> t = {};
    for (unsigned j = threadIdx.x; j < blocks; j += kFinalThreads) t.combine(slab[j]);
    if (!workgroup_reduce<kFinalThreads / 64>(t, threadIdx.x % 64, threadIdx.x / 64)) return;
    flow2d_flow_error_stats rec;
    flow2d_flow_error_class* cls[2] = {&rec.noc, &rec.occ};
    for (int k = 0; k < 2; ++k) {
        flow2d_flow_error_class& c = *cls[k];
        c.count = t.count[k][0];
        for (int i = 0; i < 4; ++i) c.above[i] = t.count[k][1 + i];
        c.fl = t.count[k][5];
        c.sum_epe = t.sum[k][0];
        c.sum_epe_sq = t.sum[k][1];
        c.sum_ae = t.sum[k][2];
        c.max_epe = static_cast<double>(t.max_epe[k]);
    }
    rec.all.count = rec.noc.count + rec.occ.count;
    for (int i = 0; i < 4; ++i) rec.all.above[i] = rec.noc.above[i] + rec.occ.above[i];
    rec.all.fl = rec.noc.fl + rec.occ.fl;
    rec.all.sum_epe = rec.noc.sum_epe + rec.occ.sum_epe;
    rec.all.sum_epe_sq = rec.noc.sum_epe_sq + rec.occ.sum_epe_sq;
    rec.all.sum_ae = rec.noc.sum_ae + rec.occ.sum_ae;
    rec.all.max_epe = fmax(rec.noc.max_epe, rec.occ.max_epe);
    rec.invalid_ground_truth = t.invalid;
    rec.nonfinite_estimate = t.nonfinite;
    stats[blockIdx.x] = rec;
}

inline size_t partial_blocks(size_t width, size_t height)
{
    return static_cast<size_t>(flow2d::div_up(width, kBlockCols)) * flow2d::div_up(height, kBlockRows);
}

}  // namespace

extern "C" {

size_t flow2d_flow_error_workspace_bytes(size_t width, size_t height, size_t instances)
{
    if (width == 0 || height == 0 || instances == 0) return 0;
    return partial_blocks(width, height) * instances * sizeof(FlowErrorPartial);
}

int flow2d_flow_error_2d(flow2d_context* ctx, const float* flow_u, const float* flow_v, const float* gt_u, const float* gt_v,
                         const float* occlusion, size_t width, size_t height, size_t pitch_bytes, float* epe, float* ae,
                         flow2d_flow_error_stats* stats, void* workspace, size_t workspace_bytes)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    const float* inputs[] = {flow_u, flow_v, gt_u, gt_v, occlusion};
    for (int i = 0; i < 4; ++i)
        if (!flow2d::plane_args_ok(inputs[i], width, height, pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    for (const float* p : {occlusion, static_cast<const float*>(epe), static_cast<const float*>(ae)})
        if (p && !flow2d::plane_args_ok(p, width, height, pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!stats || (reinterpret_cast<uintptr_t>(stats) % alignof(flow2d_flow_error_stats)) != 0 || !workspace ||
        (reinterpret_cast<uintptr_t>(workspace) % 16) != 0 ||
        workspace_bytes < flow2d_flow_error_workspace_bytes(width, height, 1))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    // the kernels mark every plane __restrict__: no written byte range may meet a read one or another written one
    auto aliased = [&](size_t span, size_t instances) {
        const flow2d::ByteRange written[] = {{epe, span}, {ae, span}, {stats, instances * sizeof(flow2d_flow_error_stats)},
                                             {workspace, workspace_bytes}};
        flow2d::ByteRange read[5];
        for (int i = 0; i < 5; ++i) read[i] = {inputs[i], span};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(height * pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t instances = ctx->batch_count;
    if (workspace_bytes < flow2d_flow_error_workspace_bytes(width, height, instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (aliased(flow2d::batch_span(ctx, height * pitch_bytes), instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    const dim3 grid(flow2d::div_up(width, kBlockCols), flow2d::div_up(height, kBlockRows), flow2d::batch_z(ctx, 1));
    const BatchArg batch = flow2d::batch_arg(ctx, 1);
    FlowErrorPartial* partials = static_cast<FlowErrorPartial*>(workspace);
    const int w = static_cast<int>(width), h = static_cast<int>(height), pitch = static_cast<int>(pitch_bytes / 4);
    // (the largest offset a lane forms is below height * pitch floats: taking the bytes leaves a margin)
    flow2d::launch_by_span(height * pitch_bytes, [&](auto offset) {
        using Offset = decltype(offset);
        const dim3 block(kLanesX, kWavesY);
        if (occlusion)
            flow_error_partials_kernel<Offset, true><<<grid, block, 0, ctx->stream>>>(flow_u, flow_v, gt_u, gt_v, occlusion, w, h,
                                                                                     pitch, epe, ae, partials, batch);
        else
            flow_error_partials_kernel<Offset, false><<<grid, block, 0, ctx->stream>>>(flow_u, flow_v, gt_u, gt_v, nullptr, w, h,
                                                                                      pitch, epe, ae, partials, batch);
    });
    FLOW2D_CHECK_LAUNCH();
    flow_error_final_kernel<<<dim3(static_cast<unsigned>(instances)), dim3(kFinalThreads), 0, ctx->stream>>>(
        partials, static_cast<unsigned>(partial_blocks(width, height)), stats);
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"

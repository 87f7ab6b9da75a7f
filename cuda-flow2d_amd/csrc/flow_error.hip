// Error statistics of a flow estimate against ground truth for gfx950: no reference counterpart.
//
// Per pixel the endpoint error, the angular error and the class of flow2d_flow_error_2d (normative definition in
// flow2d_c_abi.h), summed into one record per lock-step instance.  Built -ffp-contract=off: the EPE plane follows that
// definition bit for bit.
//
// Memory-bound: 16 bytes of flow and ground truth per pixel (20 with an occlusion plane), read as dwordx4 per lane -- a wave
// covers 256 columns of one row --, and 4 bytes per per-pixel plane written.  Two launches, no atomics: every workgroup
// reduces its 256 x 32 pixels in a fixed order (rows, then the four columns of a lane, then a lane butterfly, then the four
// waves) into a slab of the workspace, and one workgroup per instance sums the slabs in block order.  The grid, and with it
// the order of every double addition, depends only on (width, height): repeated calls and batch instances give the same bytes.
#include <cfloat>
#include <cmath>

#include "common.hpp"

namespace {

constexpr int kLanesX = 64;         // lanes of a wave along x, four columns each
constexpr int kWavesY = 4;          // waves of a workgroup, one row apart
constexpr int kRowsPerThread = 8;
constexpr int kBlockCols = kLanesX * 4;                 // 256
constexpr int kBlockRows = kWavesY * kRowsPerThread;    // 32
constexpr int kFinalThreads = 256;
constexpr float kDegrees = 57.29577951308232f;

// Per-workgroup slab: classes noc (0) and occ (1); all = noc + occ is formed by the final kernel.
struct FlowErrorPartial {
    double sum[2][3];        // epe, epe^2, ae
    float max_epe[2];
    unsigned count[2][6];    // count, above 0.5 / 1 / 2 / 3, fl
    unsigned invalid, nonfinite;
};
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

template <typename T>
__device__ __forceinline__ T wave_sum(T x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__device__ __forceinline__ float wave_max(float x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
    return x;
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
    // lane butterfly (every lane ends with the same bits: IEEE addition commutes), then the four waves in order
    __shared__ FlowErrorPartial waves[kWavesY];
    const int lane = threadIdx.x;
    FlowErrorPartial mine;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const ClassAcc& c = k ? acc.occ : acc.noc;
        mine.sum[k][0] = wave_sum(c.s_epe);
        mine.sum[k][1] = wave_sum(c.s_epe_sq);
        mine.sum[k][2] = wave_sum(c.s_ae);
        mine.max_epe[k] = wave_max(c.max_epe);
        mine.count[k][0] = wave_sum(c.n);
        mine.count[k][1] = wave_sum(c.a05);
        mine.count[k][2] = wave_sum(c.a1);
        mine.count[k][3] = wave_sum(c.a2);
        mine.count[k][4] = wave_sum(c.a3);
        mine.count[k][5] = wave_sum(c.fl);
    }
    mine.invalid = wave_sum(acc.invalid);
    mine.nonfinite = wave_sum(acc.nonfinite);
    if (lane == 0) waves[threadIdx.y] = mine;
    __syncthreads();
    if (threadIdx.y == 0 && lane == 0) {
        FlowErrorPartial out = waves[0];
        for (int wv = 1; wv < kWavesY; ++wv) {
            const FlowErrorPartial& q = waves[wv];
            for (int k = 0; k < 2; ++k) {
                for (int j = 0; j < 3; ++j) out.sum[k][j] += q.sum[k][j];
                out.max_epe[k] = fmaxf(out.max_epe[k], q.max_epe[k]);
                for (int j = 0; j < 6; ++j) out.count[k][j] += q.count[k][j];
            }
            out.invalid += q.invalid;
            out.nonfinite += q.nonfinite;
        }
        partials[static_cast<size_t>(blockIdx.z) * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] = out;
    }
}

struct FinalAcc {
    double sum[2][3];
    float max_epe[2];
    unsigned long long count[2][6];
    unsigned long long invalid, nonfinite;
};

// One workgroup per instance: thread t sums slabs t, t + 256, ... in order, then a lane butterfly and the four waves in order.
__global__ __launch_bounds__(kFinalThreads) void flow_error_final_kernel(const FlowErrorPartial* __restrict__ partials,
                                                                         unsigned blocks, flow2d_flow_error_stats* __restrict__ stats)
{
    const FlowErrorPartial* slab = partials + static_cast<size_t>(blockIdx.x) * blocks;
    FinalAcc a = {};
    for (unsigned j = threadIdx.x; j < blocks; j += kFinalThreads) {
        const FlowErrorPartial& q = slab[j];
        for (int k = 0; k < 2; ++k) {
            for (int i = 0; i < 3; ++i) a.sum[k][i] += q.sum[k][i];
            a.max_epe[k] = fmaxf(a.max_epe[k], q.max_epe[k]);
            for (int i = 0; i < 6; ++i) a.count[k][i] += q.count[k][i];
        }
        a.invalid += q.invalid;
        a.nonfinite += q.nonfinite;
    }
    for (int k = 0; k < 2; ++k) {
        for (int i = 0; i < 3; ++i) a.sum[k][i] = wave_sum(a.sum[k][i]);
        a.max_epe[k] = wave_max(a.max_epe[k]);
        for (int i = 0; i < 6; ++i) a.count[k][i] = wave_sum(a.count[k][i]);
    }
    a.invalid = wave_sum(a.invalid);
    a.nonfinite = wave_sum(a.nonfinite);
    __shared__ FinalAcc waves[kFinalThreads / 64];
    const int wave = threadIdx.x / 64;
    if (threadIdx.x % 64 == 0) waves[wave] = a;
    __syncthreads();
    if (threadIdx.x != 0) return;
    FinalAcc t = waves[0];
    for (int wv = 1; wv < kFinalThreads / 64; ++wv) {
        const FinalAcc& q = waves[wv];
        for (int k = 0; k < 2; ++k) {
            for (int i = 0; i < 3; ++i) t.sum[k][i] += q.sum[k][i];
            t.max_epe[k] = fmaxf(t.max_epe[k], q.max_epe[k]);
            for (int i = 0; i < 6; ++i) t.count[k][i] += q.count[k][i];
        }
        t.invalid += q.invalid;
        t.nonfinite += q.nonfinite;
    }
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

inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + b_bytes && pb < pa + a_bytes;
}

inline size_t partial_blocks(size_t width, size_t height)
{
    return static_cast<size_t>(flow2d::div_up(width, kBlockCols)) * flow2d::div_up(height, kBlockRows);
}

// The written ranges (epe, ae: `plane` bytes each; stats, workspace) against every read plane and each other.
bool outputs_overlap(const float* const* inputs, int n_inputs, const float* epe, const float* ae, size_t plane,
                     const void* stats, size_t stats_bytes, const void* workspace, size_t workspace_bytes)
{
    const float* outs[2] = {epe, ae};
    for (const float* o : outs) {
        if (!o) continue;
        for (int i = 0; i < n_inputs; ++i)
            if (inputs[i] && ranges_overlap(o, plane, inputs[i], plane)) return true;
        if (ranges_overlap(o, plane, stats, stats_bytes) || ranges_overlap(o, plane, workspace, workspace_bytes)) return true;
    }
    if (epe && ae && ranges_overlap(epe, plane, ae, plane)) return true;
    for (int i = 0; i < n_inputs; ++i)
        if (inputs[i] && (ranges_overlap(stats, stats_bytes, inputs[i], plane) ||
                          ranges_overlap(workspace, workspace_bytes, inputs[i], plane)))
            return true;
    return ranges_overlap(stats, stats_bytes, workspace, workspace_bytes);
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
    if (outputs_overlap(inputs, 5, epe, ae, height * pitch_bytes, stats, sizeof(flow2d_flow_error_stats), workspace,
                        workspace_bytes))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t instances = ctx->batch_count;
    if (workspace_bytes < flow2d_flow_error_workspace_bytes(width, height, instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    // a lock-step batch: instance b of every plane at + b * stride, so each plane spans all instances
    const size_t span = height * pitch_bytes + (instances - 1) * ctx->batch_stride_floats * sizeof(float);
    if (outputs_overlap(inputs, 5, epe, ae, span, stats, instances * sizeof(flow2d_flow_error_stats), workspace,
                        workspace_bytes))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    const dim3 grid(flow2d::div_up(width, kBlockCols), flow2d::div_up(height, kBlockRows), flow2d::batch_z(ctx, 1));
    const BatchArg batch = flow2d::batch_arg(ctx, 1);
    FlowErrorPartial* partials = static_cast<FlowErrorPartial*>(workspace);
    const int w = static_cast<int>(width), h = static_cast<int>(height), pitch = static_cast<int>(pitch_bytes / 4);
    // 32-bit per-lane offsets when the largest one a lane forms -- below height * pitch floats -- fits (bytes: a margin)
    const bool small = height * pitch_bytes < (size_t(1) << 32);
    const dim3 block(kLanesX, kWavesY);
    if (occlusion) {
        if (small)
            flow_error_partials_kernel<unsigned, true><<<grid, block, 0, ctx->stream>>>(flow_u, flow_v, gt_u, gt_v, occlusion, w, h,
                                                                                       pitch, epe, ae, partials, batch);
        else
            flow_error_partials_kernel<size_t, true><<<grid, block, 0, ctx->stream>>>(flow_u, flow_v, gt_u, gt_v, occlusion, w, h,
                                                                                     pitch, epe, ae, partials, batch);
    } else {
        if (small)
            flow_error_partials_kernel<unsigned, false><<<grid, block, 0, ctx->stream>>>(flow_u, flow_v, gt_u, gt_v, nullptr, w, h,
                                                                                        pitch, epe, ae, partials, batch);
        else
            flow_error_partials_kernel<size_t, false><<<grid, block, 0, ctx->stream>>>(flow_u, flow_v, gt_u, gt_v, nullptr, w, h,
                                                                                      pitch, epe, ae, partials, batch);
    }
    FLOW2D_CHECK_LAUNCH();
    flow_error_final_kernel<<<dim3(static_cast<unsigned>(instances)), dim3(kFinalThreads), 0, ctx->stream>>>(
        partials, static_cast<unsigned>(partial_blocks(width, height)), stats);
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"

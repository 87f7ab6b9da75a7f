// Robust global motion of a flow field for gfx950: no reference counterpart.
//
// flow2d_global_motion_2d: a translation, similarity or affine motion of the whole frame fitted to a flow by iteratively
// reweighted least squares; flow2d_global_flow_2d: that model as planes, the residual flow and the inlier map;
// flow2d_warp_global_2d: a frame resampled along a model (stabilisation).  The normative definitions are those of the three
// entries in flow2d_c_abi.h.  The fit and the model are IEEE double (full rate on this chip), built -ffp-contract=off: the
// only difference to a restatement is the order of the twelve sums.  The bilinear sample is the operation order of
// flow2d_consistency_2d (consistency.hip).
//
// The fit is memory-bound and has the geometry of flow_error.hip: 8 bytes of flow per pixel (12 with a mask) read as dwordx4
// per lane -- a wave covers 256 columns of one row --, per pass two launches and no atomics: every workgroup reduces its
// 256 x 32 pixels in a fixed order (rows, then the four columns of a lane, then a lane butterfly, then the four waves) into a
// slab of the workspace, and one workgroup per instance sums the slabs in block order, solves and writes the record.  The next
// pass reads that record from device memory (uniform loads: scalar registers).  The grid, and with it the order of every
// addition, depends only on (width, height): repeated calls and batch instances give the same bytes.
// The per-pixel kernels have the geometry and the sampler of plane_sample.hpp: 64 x 4 threads, four rows per thread, one byte
// offset per lane (32 bits when the plane's span allows) against scalar bases, column-pair dwordx2 gathers; the warp reads no
// flow plane.
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
constexpr int kSums = 12;  // S0 Sx Sy Sxx Sxy Syy Su Sxu Syu Sv Sxv Syv
constexpr int kPlaneRows = 4;  // rows per thread of the per-pixel kernels
constexpr unsigned kQuietNaN = 0x7fc00000u;

struct MotionPartial {
    double s[kSums];
    unsigned long long support;
    unsigned long long reserved;
};
static_assert(sizeof(MotionPartial) % 16 == 0, "slabs stay 16-byte aligned");

struct Model {
    double p0, p1, p2, p3, p4, p5;
};

// (uniform address: the six parameters land in scalar registers)
__device__ __forceinline__ Model load_model(const flow2d_global_motion* __restrict__ rec)
{
    return Model{rec->p[0], rec->p[1], rec->p[2], rec->p[3], rec->p[4], rec->p[5]};
}

__device__ __forceinline__ double model_u(const Model& m, double xc, double yc) { return (m.p0 + m.p1 * xc) + m.p2 * yc; }
__device__ __forceinline__ double model_v(const Model& m, double xc, double yc) { return (m.p3 + m.p4 * xc) + m.p5 * yc; }

__device__ __forceinline__ float clamp_mask(float m)
{
    if (!(m <= 1.f)) m = 1.f;  // NaN: left out
    if (!(m >= 0.f)) m = 0.f;
    return m;
}

__device__ __forceinline__ bool flow_valid(float u, float v) { return fabsf(u) <= 1e9f && fabsf(v) <= 1e9f; }  // NaN, inf fail

struct Acc {
    double s[kSums] = {};
    unsigned support = 0;
};

// One pixel of the definition.  Weighted: a pass after the first, with the record of the pass before.
template <bool Weighted>
__device__ __forceinline__ void fit_pixel(float uf, float vf, float mf, double xc, double yc, const Model& model, double s2,
                                          Acc& a)
{
    const bool valid = flow_valid(uf, vf);
    const double b = valid ? static_cast<double>(1.f - clamp_mask(mf)) : 0.0;
    const double u = valid ? static_cast<double>(uf) : 0.0, v = valid ? static_cast<double>(vf) : 0.0;
    double w = b;
    if (Weighted) {
        const double du = u - model_u(model, xc, yc), dv = v - model_v(model, xc, yc);
        w = b * (s2 / (s2 + (du * du + dv * dv)));
    }
    a.support += b > 0.0;
    const double wx = w * xc, wy = w * yc;
    a.s[0] += w;
    a.s[1] += wx;
    a.s[2] += wy;
    a.s[3] += wx * xc;
    a.s[4] += wx * yc;
    a.s[5] += wy * yc;
    a.s[6] += w * u;
    a.s[7] += wx * u;
    a.s[8] += wy * u;
    a.s[9] += w * v;
    a.s[10] += wx * v;
    a.s[11] += wy * v;
}

// Offset: unsigned (a plane's whole extent fits 32 bits) or size_t; HasMask: a mask plane is read; Weighted: see fit_pixel.
template <typename Offset, bool HasMask, bool Weighted>
__global__ __launch_bounds__(256) void motion_partials_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                              const float* __restrict__ mask, int w, int h, int pitch,
                                                              const flow2d_global_motion* __restrict__ previous, double s2,
                                                              MotionPartial* __restrict__ partials, BatchArg batch)
{
    const size_t inst = batch_offset(batch);
    u += inst;
    v += inst;
    if (HasMask) mask += inst;
    Model model = {};
    if (Weighted) model = load_model(previous + blockIdx.z);
    const double cx = static_cast<double>(w - 1) * 0.5, cy = static_cast<double>(h - 1) * 0.5;
    const int x0 = (blockIdx.x * kLanesX + threadIdx.x) * 4;
    Acc acc;
    if (x0 < w) {
        const double xc = static_cast<double>(x0) - cx;
        const int n = min(4, w - x0);
#pragma unroll 2
        for (int i = 0; i < kRowsPerThread; ++i) {
            const int gy = blockIdx.y * kBlockRows + i * kWavesY + threadIdx.y;
            if (gy >= h) break;
            // x0 < w and the pitch is a multiple of four floats: the four columns lie inside the row, padding included
            const Offset c = static_cast<Offset>(gy) * static_cast<Offset>(pitch) + static_cast<Offset>(x0);
            const float4 fu = *reinterpret_cast<const float4*>(u + c);
            const float4 fv = *reinterpret_cast<const float4*>(v + c);
            float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
            if (HasMask) m = *reinterpret_cast<const float4*>(mask + c);
            const double yc = static_cast<double>(gy) - cy;
            // the columns beyond the width are row padding: they take no part
            fit_pixel<Weighted>(fu.x, fv.x, m.x, xc, yc, model, s2, acc);
            if (n > 1) fit_pixel<Weighted>(fu.y, fv.y, m.y, xc + 1.0, yc, model, s2, acc);
            if (n > 2) fit_pixel<Weighted>(fu.z, fv.z, m.z, xc + 2.0, yc, model, s2, acc);
            if (n > 3) fit_pixel<Weighted>(fu.w, fv.w, m.w, xc + 3.0, yc, model, s2, acc);
        }
    }
    // lane butterfly (every lane ends with the same bits: IEEE addition commutes), then the four waves in order.  The steps of
    // workgroup_reduce (ordered_reduce.hpp), kept spelled out here and in motion_final_kernel: see that header.
    __shared__ MotionPartial waves[kWavesY];
    MotionPartial mine;
#pragma unroll
    for (int j = 0; j < kSums; ++j) mine.s[j] = wave_sum(acc.s[j]);
    mine.support = wave_sum(acc.support);
    mine.reserved = 0;
    if (threadIdx.x == 0) waves[threadIdx.y] = mine;
    __syncthreads();
    if (threadIdx.y == 0 && threadIdx.x == 0) {
        MotionPartial out = waves[0];
        for (int wv = 1; wv < kWavesY; ++wv) {
            for (int j = 0; j < kSums; ++j) out.s[j] += waves[wv].s[j];
            out.support += waves[wv].support;
        }
        partials[static_cast<size_t>(blockIdx.z) * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] = out;
    }
}

// The solve of the definition, operation for operation.
__device__ void solve_motion(const double (&s)[kSums], int model, flow2d_global_motion& rec)
{
    for (double& q : rec.p) q = 0.0;
    rec.weight_sum = s[0];
    rec.model_used = -1;
    const double s0 = s[0];
    if (!(s0 > 0.0)) return;
    const double mx = s[1] / s0, my = s[2] / s0, mu = s[6] / s0, mv = s[9] / s0;
    const double cxx = s[3] / s0 - mx * mx, cxy = s[4] / s0 - mx * my, cyy = s[5] / s0 - my * my;
    const double cxu = s[7] / s0 - mx * mu, cyu = s[8] / s0 - my * mu;
    const double cxv = s[10] / s0 - mx * mv, cyv = s[11] / s0 - my * mv;
    const double spread = cxx + cyy, det = cxx * cyy - cxy * cxy;
    int used = model;
    if (used == FLOW2D_MOTION_AFFINE && !(spread > 1e-9 && det > 1e-9 * (spread * spread))) used = FLOW2D_MOTION_SIMILARITY;
    if (used == FLOW2D_MOTION_SIMILARITY && !(spread > 1e-9)) used = FLOW2D_MOTION_TRANSLATION;
    double p1 = 0.0, p2 = 0.0, p4 = 0.0, p5 = 0.0;
    if (used == FLOW2D_MOTION_AFFINE) {
        p1 = (cxu * cyy - cyu * cxy) / det;
        p2 = (cyu * cxx - cxu * cxy) / det;
        p4 = (cxv * cyy - cyv * cxy) / det;
        p5 = (cyv * cxx - cxv * cxy) / det;
    } else if (used == FLOW2D_MOTION_SIMILARITY) {
        const double a = (cxu + cyv) / spread, b = (cxv - cyu) / spread;
        p1 = a;
        p2 = -b;
        p4 = b;
        p5 = a;
    }
    rec.p[0] = mu - (p1 * mx + p2 * my);
    rec.p[1] = p1;
    rec.p[2] = p2;
    rec.p[3] = mv - (p4 * mx + p5 * my);
    rec.p[4] = p4;
    rec.p[5] = p5;
    rec.model_used = used;
}

// One workgroup per instance: thread t sums slabs t, t + 256, ... in order, then a lane butterfly and the four waves in order.
__global__ __launch_bounds__(kFinalThreads) void motion_final_kernel(const MotionPartial* __restrict__ partials, unsigned blocks,
                                                                     int model, flow2d_global_motion* __restrict__ motion)
{
    const MotionPartial* slab = partials + static_cast<size_t>(blockIdx.x) * blocks;
    double s[kSums] = {};
    unsigned long long support = 0;
    for (unsigned j = threadIdx.x; j < blocks; j += kFinalThreads) {
#pragma unroll
        for (int i = 0; i < kSums; ++i) s[i] += slab[j].s[i];
        support += slab[j].support;
    }
#pragma unroll
    for (int i = 0; i < kSums; ++i) s[i] = wave_sum(s[i]);
    support = wave_sum(support);
    __shared__ MotionPartial waves[kFinalThreads / 64];
    const int wave = threadIdx.x / 64;
    if (threadIdx.x % 64 == 0) {
#pragma unroll
        for (int i = 0; i < kSums; ++i) waves[wave].s[i] = s[i];
        waves[wave].support = support;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int wv = 1; wv < kFinalThreads / 64; ++wv) {
#pragma unroll
        for (int i = 0; i < kSums; ++i) s[i] += waves[wv].s[i];
        support += waves[wv].support;
    }
    flow2d_global_motion rec;
    solve_motion(s, model, rec);
    rec.support = support;
    rec.reserved[0] = rec.reserved[1] = rec.reserved[2] = 0;
    motion[blockIdx.x] = rec;
}

__device__ __forceinline__ float canonical_nan(float r)
{
    const unsigned bits = __float_as_uint(r);
    return (bits & 0x7fffffffu) > 0x7f800000u ? __uint_as_float(kQuietNaN) : r;
}

// The model as planes, the residual flow and the inlier map.  HasFlow: the flow planes are read (residual, weight).
template <typename Offset, bool HasFlow>
__global__ __launch_bounds__(256) void global_flow_kernel(const flow2d_global_motion* __restrict__ motion,
                                                          const float* __restrict__ u, const float* __restrict__ v,
                                                          const float* __restrict__ mask, int w, int h, int pitch, double s2,
                                                          float* __restrict__ out_mu, float* __restrict__ out_mv,
                                                          float* __restrict__ res_u, float* __restrict__ res_v,
                                                          float* __restrict__ weight, BatchArg batch)
{
    const size_t inst = batch_offset(batch);
    const Model model = load_model(motion + blockIdx.z);
    const int gx = pixel_column();
    if (gx >= w) return;
    const double xc = static_cast<double>(gx) - static_cast<double>(w - 1) * 0.5;
    const double cy = static_cast<double>(h - 1) * 0.5;
#pragma unroll
    for (int i = 0; i < kPlaneRows; ++i) {
        const int gy = pixel_row(kPlaneRows, i);
        if (gy >= h) return;
        const Offset at = pixel_offset<Offset>(gx, gy, pitch);
        const double yc = static_cast<double>(gy) - cy;
        const double mu = model_u(model, xc, yc), mv = model_v(model, xc, yc);
        if (out_mu) {
            store_at(out_mu + inst, at, canonical_nan(static_cast<float>(mu)));
            store_at(out_mv + inst, at, canonical_nan(static_cast<float>(mv)));
        }
        if (HasFlow) {
            const float uf = load_at(u + inst, at), vf = load_at(v + inst, at);
            const bool valid = flow_valid(uf, vf);
            const double ud = valid ? static_cast<double>(uf) : 0.0, vd = valid ? static_cast<double>(vf) : 0.0;
            const double du = ud - mu, dv = vd - mv;
            if (res_u) {
                const float nan = __uint_as_float(kQuietNaN);
                store_at(res_u + inst, at, valid ? canonical_nan(static_cast<float>(du)) : nan);
                store_at(res_v + inst, at, valid ? canonical_nan(static_cast<float>(dv)) : nan);
            }
            if (weight) {
                const float m = mask ? load_at(mask + inst, at) : 0.f;
                const double b = valid ? static_cast<double>(1.f - clamp_mask(m)) : 0.0;
                const double wgt = s2 > 0.0 ? b * (s2 / (s2 + (du * du + dv * dv))) : b;
                store_at(weight + inst, at, canonical_nan(static_cast<float>(wgt)));
            }
        }
    }
}

// One frame resampled along the model: the sample of consistency_kernel at q = x + model(x).
template <typename Offset>
__global__ __launch_bounds__(256) void warp_global_kernel(const flow2d_global_motion* __restrict__ motion,
                                                          const float* __restrict__ frame, int w, int h, int pitch, float fill,
                                                          float* __restrict__ output, float* __restrict__ valid, BatchArg batch)
{
    const size_t inst = batch_offset(batch);
    frame += inst;
    output += inst;
    if (valid) valid += inst;
    const Model model = load_model(motion + blockIdx.z);
    const int gx = pixel_column();
    if (gx >= w) return;
    const double xd = static_cast<double>(gx), xc = xd - static_cast<double>(w - 1) * 0.5;
    const double cy = static_cast<double>(h - 1) * 0.5;
    const float x_max = static_cast<float>(w - 1), y_max = static_cast<float>(h - 1);

    // every position and gather first (rows past the frame run on the last row and write nothing), then the blends
    Offset at[kPlaneRows];
    Tap<Offset> tap[kPlaneRows];
    float2 ga[kPlaneRows], gb[kPlaneRows];
    bool ok[kPlaneRows];
#pragma unroll
    for (int i = 0; i < kPlaneRows; ++i) {
        const int gy = min(pixel_row(kPlaneRows, i), h - 1);
        at[i] = pixel_offset<Offset>(gx, gy, pitch);
        const double yd = static_cast<double>(gy), yc = yd - cy;
        float qx = static_cast<float>(xd + model_u(model, xc, yc));
        float qy = static_cast<float>(yd + model_v(model, xc, yc));
        ok[i] = qx >= 0.f && qx <= x_max && qy >= 0.f && qy <= y_max;  // a NaN or an infinity fails
        if (!ok[i]) {  // sampled at the pixel itself and not used
            qx = static_cast<float>(gx);
            qy = static_cast<float>(gy);
        }
        tap[i] = make_tap<Offset>(qx, qy, w, h, pitch);
        ga[i] = column_pair(frame, tap[i].o0);
        gb[i] = column_pair(frame, tap[i].o1);
    }
#pragma unroll
    for (int i = 0; i < kPlaneRows; ++i) {
        const int gy = pixel_row(kPlaneRows, i);
        if (gy >= h) return;
        const float s = blend(tap[i], ga[i], gb[i]);
        store_at(output, at[i], ok[i] ? s : fill);
        if (valid) store_at(valid, at[i], ok[i] ? 1.f : 0.f);
    }
}

inline size_t partial_blocks(size_t width, size_t height)
{
    return static_cast<size_t>(flow2d::div_up(width, kBlockCols)) * flow2d::div_up(height, kBlockRows);
}

inline bool record_ok(const void* motion) { return motion && (reinterpret_cast<uintptr_t>(motion) % 8) == 0; }

template <typename Offset>
void launch_partials(flow2d_context* ctx, dim3 grid, const float* u, const float* v, const float* mask, int w, int h, int pitch,
                     const flow2d_global_motion* previous, double s2, MotionPartial* partials, BatchArg batch)
{
    const dim3 block(kLanesX, kWavesY);
#define FLOW2D_MOTION_LAUNCH(HAS_MASK, WEIGHTED)                                                                          \
    motion_partials_kernel<Offset, HAS_MASK, WEIGHTED><<<grid, block, 0, ctx->stream>>>(u, v, mask, w, h, pitch, previous, s2, \
                                                                                        partials, batch)
    if (mask) {
        if (previous)
            FLOW2D_MOTION_LAUNCH(true, true);
        else
            FLOW2D_MOTION_LAUNCH(true, false);
    } else {
        if (previous)
            FLOW2D_MOTION_LAUNCH(false, true);
        else
            FLOW2D_MOTION_LAUNCH(false, false);
    }
#undef FLOW2D_MOTION_LAUNCH
}

}  // namespace

extern "C" {

size_t flow2d_global_motion_workspace_bytes(size_t width, size_t height, size_t instances)
{
    if (width == 0 || height == 0 || instances == 0) return 0;
    return partial_blocks(width, height) * instances * sizeof(MotionPartial);
}

int flow2d_global_motion_2d(flow2d_context* ctx, const float* flow_u, const float* flow_v, const float* mask, size_t width,
                            size_t height, size_t pitch_bytes, int model, double sigma, int iterations,
                            flow2d_global_motion* motion, void* workspace, size_t workspace_bytes)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    if (!flow2d::plane_args_ok(flow_u, width, height, pitch_bytes) || !flow2d::plane_args_ok(flow_v, width, height, pitch_bytes) ||
        (mask && !flow2d::plane_args_ok(mask, width, height, pitch_bytes)))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (model != FLOW2D_MOTION_TRANSLATION && model != FLOW2D_MOTION_SIMILARITY && model != FLOW2D_MOTION_AFFINE)
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(sigma) || sigma < 0.0 || iterations < 0 || iterations > FLOW2D_GLOBAL_MOTION_MAX_ITERATIONS)
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!record_ok(motion) || !workspace || (reinterpret_cast<uintptr_t>(workspace) % 16) != 0 ||
        workspace_bytes < flow2d_global_motion_workspace_bytes(width, height, 1))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    auto aliased = [&](size_t span, size_t instances) {
        const flow2d::ByteRange written[] = {{motion, instances * sizeof(flow2d_global_motion)}, {workspace, workspace_bytes}};
        const flow2d::ByteRange read[] = {{flow_u, span}, {flow_v, span}, {mask, span}};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(height * pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t instances = ctx->batch_count;
    if (workspace_bytes < flow2d_global_motion_workspace_bytes(width, height, instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (aliased(flow2d::batch_span(ctx, height * pitch_bytes), instances))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    const dim3 grid(flow2d::div_up(width, kBlockCols), flow2d::div_up(height, kBlockRows), flow2d::batch_z(ctx, 1));
    const BatchArg batch = flow2d::batch_arg(ctx, 1);
    MotionPartial* partials = static_cast<MotionPartial*>(workspace);
    const int w = static_cast<int>(width), h = static_cast<int>(height), pitch = static_cast<int>(pitch_bytes / 4);
    const unsigned blocks = static_cast<unsigned>(partial_blocks(width, height));
    const double s2 = sigma * sigma;
    const int passes = 1 + (sigma > 0.0 ? iterations : 0);
    for (int pass = 0; pass < passes; ++pass) {
        const flow2d_global_motion* previous = pass > 0 ? motion : nullptr;
        // (the largest offset a lane forms is below height * pitch floats: taking the bytes leaves a margin)
        flow2d::launch_by_span(height * pitch_bytes, [&](auto offset) {
            launch_partials<decltype(offset)>(ctx, grid, flow_u, flow_v, mask, w, h, pitch, previous, s2, partials, batch);
        });
        FLOW2D_CHECK_LAUNCH();
        motion_final_kernel<<<dim3(static_cast<unsigned>(instances)), dim3(kFinalThreads), 0, ctx->stream>>>(partials, blocks,
                                                                                                             model, motion);
        FLOW2D_CHECK_LAUNCH();
    }
    return FLOW2D_OK;
}

int flow2d_global_flow_2d(flow2d_context* ctx, const flow2d_global_motion* motion, const float* flow_u, const float* flow_v,
                          const float* mask, size_t width, size_t height, size_t pitch_bytes, double sigma, float* model_u,
                          float* model_v, float* residual_u, float* residual_v, float* weight)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    if (!record_ok(motion) || !std::isfinite(sigma) || sigma < 0.0) return FLOW2D_ERR_INVALID_ARGUMENT;
    if ((flow_u == nullptr) != (flow_v == nullptr) || (model_u == nullptr) != (model_v == nullptr) ||
        (residual_u == nullptr) != (residual_v == nullptr))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!model_u && !residual_u && !weight) return FLOW2D_ERR_INVALID_ARGUMENT;
    if ((residual_u || weight) && !flow_u) return FLOW2D_ERR_INVALID_ARGUMENT;
    const float* inputs[] = {flow_u, flow_v, mask};
    float* const written[] = {model_u, model_v, residual_u, residual_v, weight};
    if (width == 0 || height == 0) return FLOW2D_ERR_INVALID_ARGUMENT;
    for (const float* p : inputs)
        if (p && !flow2d::plane_args_ok(p, width, height, pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    for (const float* p : written)
        if (p && !flow2d::plane_args_ok(p, width, height, pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    auto aliased = [&](size_t span, size_t instances) {
        flow2d::ByteRange out[5], in[4];
        for (int i = 0; i < 5; ++i) out[i] = flow2d::ByteRange{written[i], span};
        for (int i = 0; i < 3; ++i) in[i] = flow2d::ByteRange{inputs[i], span};
        in[3] = flow2d::ByteRange{motion, instances * sizeof(flow2d_global_motion)};
        return flow2d::any_overlap(out, in);
    };
    if (aliased(height * pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    if (aliased(flow2d::batch_span(ctx, height * pitch_bytes), ctx->batch_count))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    const dim3 grid = flow2d::pixel_grid(ctx, width, height, kPlaneRows);
    const BatchArg batch = flow2d::batch_arg(ctx, 1);
    const int w = static_cast<int>(width), h = static_cast<int>(height), pitch = static_cast<int>(pitch_bytes / 4);
    const double s2 = sigma * sigma;
    flow2d::launch_by_span(height * pitch_bytes, [&](auto offset) {
        using Offset = decltype(offset);
#define FLOW2D_GLOBAL_FLOW_LAUNCH(HAS_FLOW)                                                                                 \
    global_flow_kernel<Offset, HAS_FLOW><<<grid, flow2d::pixel_block(), 0, ctx->stream>>>(                                  \
        motion, flow_u, flow_v, mask, w, h, pitch, s2, model_u, model_v, residual_u, residual_v, weight, batch)
        if (flow_u && (residual_u || weight))
            FLOW2D_GLOBAL_FLOW_LAUNCH(true);
        else
            FLOW2D_GLOBAL_FLOW_LAUNCH(false);
#undef FLOW2D_GLOBAL_FLOW_LAUNCH
    });
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

int flow2d_warp_global_2d(flow2d_context* ctx, const flow2d_global_motion* motion, const float* frame, size_t width,
                          size_t height, size_t pitch_bytes, float fill, float* output, float* valid)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    if (!record_ok(motion) || !flow2d::plane_args_ok(frame, width, height, pitch_bytes) ||
        !flow2d::plane_args_ok(output, width, height, pitch_bytes) ||
        (valid && !flow2d::plane_args_ok(valid, width, height, pitch_bytes)))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    auto aliased = [&](size_t span, size_t instances) {
        const flow2d::ByteRange out[] = {{output, span}, {valid, span}};
        const flow2d::ByteRange in[] = {{frame, span}, {motion, instances * sizeof(flow2d_global_motion)}};
        return flow2d::any_overlap(out, in);
    };
    if (aliased(height * pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    if (aliased(flow2d::batch_span(ctx, height * pitch_bytes), ctx->batch_count))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    flow2d::launch_by_span(height * pitch_bytes, [&](auto offset) {
        warp_global_kernel<decltype(offset)><<<flow2d::pixel_grid(ctx, width, height, kPlaneRows), flow2d::pixel_block(), 0,
                                               ctx->stream>>>(motion, frame, (int)width, (int)height, (int)(pitch_bytes / 4), fill,
                                                              output, valid, flow2d::batch_arg(ctx, 1));
    });
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"

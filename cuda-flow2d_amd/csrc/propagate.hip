// A flow carried along itself onto the next frame's grid, for gfx950: no reference counterpart (the reference runs every pair of
// a sequence from zero).  The prior of a warm-started sequence: flow k of the pair (k, k + 1) lives on frame k's grid, the prior of
// the pair (k + 1, k + 2) has to live on frame k + 1's, where the content of pixel p has moved to p + flow(p).
//
// A deterministic forward splat.  The normative definition is the one of flow2d_propagate_flow_2d in flow2d_c_abi.h; built
// -ffp-contract=off, the bits follow it exactly.  Three kinds of launch:
//   splat    every usable source pixel forms the 64-bit key of its landing (photometric match, distance to the target's centre,
//            source index) and offers it to the target's word of the workspace with ONE integer atomic max.  Max commutes and
//            associates: the word ends as the largest key offered, whatever the order of the waves.
//   resolve  every target reads its word, finds the source index in the low half and copies that source's vector; no winner: NaN.
//   fill     per pass, a hole with a finite neighbour among its eight takes their mean; the passes ping-pong between the output
//            planes and two dense planes of the workspace so that no pass reads what it writes.
//
// Memory-bound.  Splat: 8 bytes of flow per pixel (12 with a mask, 16 + four gathers with frames) and one 8-byte atomic, the
// targets of a wave near-contiguous for a smooth flow; resolve: 8 bytes of keys, a gather of 8 and a store of 8; a fill pass is a
// copy of both planes (16 bytes) with eight more loads per hole.  Geometry of the analysis kernels: 64 x 4 threads, four rows per
// thread one workgroup height apart.  Counts are summed over the wave and added by one 64-bit integer atomic per wave and counter
// that has any: the record does not depend on the order of the waves.
#include <cfloat>
#include <cmath>

#include "plane_sample.hpp"

namespace {

constexpr int kPropagateRows = 4;  // rows per thread
constexpr float kDistanceScale = 4194304.0f;  // 2^22: d2 <= 0.5 stays below 2^23
constexpr unsigned kDistanceMax = 0x7FFFFFu;

enum RecordSlot { kPixels = 0, kUnusable, kLeft, kLanded, kHoles, kFilled, kUnfilled, kReserved, kRecordSlots };
static_assert(kRecordSlots * sizeof(unsigned long long) == FLOW2D_PROPAGATE_RECORD_BYTES, "flow2d propagate record layout");

__device__ __forceinline__ bool both_finite(float a, float b) { return fabsf(a) <= FLT_MAX && fabsf(b) <= FLT_MAX; }  // false for a NaN

// the sum of a count over the wave (a wave is one row of the 64 x 4 workgroup), added by its first lane
__device__ __forceinline__ void wave_add(unsigned long long* slot, unsigned count)
{
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) count += __shfl_xor(count, step);
    if (threadIdx.x == 0 && count) atomicAdd(slot, static_cast<unsigned long long>(count));
}

struct SplatArgs {
    const float *u, *v, *mask, *from, *to;
    unsigned long long* keys;    // width * height words per instance, dense
    unsigned long long* record;  // kRecordSlots counts per instance
    int w, h, pitch;
    float step, photo_scale;
};

template <typename Offset, bool HasMask, bool HasFrames>
__global__ __launch_bounds__(flow2d::kPixelBlockX* flow2d::kPixelBlockY) void propagate_splat_kernel(SplatArgs a, BatchArg batch)
{
    const size_t inst = batch_offset(batch);
    const float* __restrict__ u = a.u + inst;
    const float* __restrict__ v = a.v + inst;
    const float* __restrict__ mask = HasMask ? a.mask + inst : nullptr;
    const float* __restrict__ from = HasFrames ? a.from + inst : nullptr;
    const float* __restrict__ to = HasFrames ? a.to + inst : nullptr;
    const size_t plane = static_cast<size_t>(a.w) * static_cast<size_t>(a.h);
    unsigned long long* __restrict__ keys = a.keys + static_cast<size_t>(blockIdx.z) * plane;
    const int gx = pixel_column();
    const float x_max = static_cast<float>(a.w - 1), y_max = static_cast<float>(a.h - 1);
    unsigned pixels = 0, unusable = 0, left = 0, landed = 0;
    if (gx < a.w) {  // (no early return: every lane of the wave takes part in the sums of the counts below)
#pragma unroll
        for (int r = 0; r < kPropagateRows; ++r) {
            const int gy = static_cast<int>(pixel_row(kPropagateRows, r));
            if (gy >= a.h) break;
            ++pixels;
            const Offset o = pixel_offset<Offset>(gx, gy, a.pitch);
            const float fu = load_at(u, o), fv = load_at(v, o);
            bool usable = both_finite(fu, fv);
            if (HasMask) usable = usable && load_at(mask, o) == 0.f;  // (a NaN in the mask compares false: unusable)
            if (!usable) {
                ++unusable;
                continue;
            }
            const float lx = static_cast<float>(gx) + a.step * fu;
            const float ly = static_cast<float>(gy) + a.step * fv;
            const float tx = floorf(lx + 0.5f), ty = floorf(ly + 0.5f);
            // compared as floats: a NaN, an infinity or a vector of 1e30 fails here and never reaches an integer conversion
            if (!(tx >= 0.f && tx <= x_max && ty >= 0.f && ty <= y_max)) {
                ++left;
                continue;
            }
            ++landed;
            const float ex = lx - tx, ey = ly - ty;
            const float d2 = ex * ex + ey * ey;
            const unsigned dq = min(static_cast<unsigned>(d2 * kDistanceScale), kDistanceMax);
            unsigned q = 0;
            if (HasFrames) {
                // the landing point lies within half a pixel of the frame: clamped onto it
                const float qx = fminf(fmaxf(lx, 0.f), x_max), qy = fminf(fmaxf(ly, 0.f), y_max);
                const Tap<Offset> tap = make_tap<Offset>(qx, qy, a.w, a.h, a.pitch);
                const float g = blend(tap, column_pair(to, tap.o0), column_pair(to, tap.o1));
                const float diff = fabsf(load_at(from, o) - g) * a.photo_scale;
                q = !(diff <= FLT_MAX) ? 255u : (diff >= 255.f ? 255u : static_cast<unsigned>(diff));  // (diff >= 0 or NaN)
            }
            const unsigned i = static_cast<unsigned>(gy) * static_cast<unsigned>(a.w) + static_cast<unsigned>(gx);
            const unsigned long long key = (static_cast<unsigned long long>(255u - q) << 56) |
                                           (static_cast<unsigned long long>(kDistanceMax - dq) << 32) |
                                           static_cast<unsigned long long>(0xFFFFFFFFu - i);
            const size_t target = static_cast<size_t>(static_cast<int>(ty)) * static_cast<size_t>(a.w) + static_cast<size_t>(static_cast<int>(tx));
            atomicMax(keys + target, key);
        }
    }
    if (a.record == nullptr) return;  // (uniform: the caller asked for no counts)
    unsigned long long* record = a.record + static_cast<size_t>(blockIdx.z) * kRecordSlots;
    wave_add(record + kPixels, pixels);
    wave_add(record + kUnusable, unusable);
    wave_add(record + kLeft, left);
    wave_add(record + kLanded, landed);
}

struct PlanePair {
    float *u, *v;
    int pitch;              // floats
    unsigned long long stride;  // floats between instances
};
struct ConstPlanePair {
    const float *u, *v;
    int pitch;
    unsigned long long stride;
};

// Every target takes its winner's vector bit for bit, or the quiet NaN 0x7fc00000 in both planes.
template <typename Offset>
__global__ __launch_bounds__(flow2d::kPixelBlockX* flow2d::kPixelBlockY) void propagate_resolve_kernel(
    const unsigned long long* __restrict__ keys_base, ConstPlanePair src, PlanePair dst, unsigned long long* record_base, int w, int h,
    int count_unfilled)
{
    const size_t plane = static_cast<size_t>(w) * static_cast<size_t>(h);
    const unsigned long long* __restrict__ keys = keys_base + static_cast<size_t>(blockIdx.z) * plane;
    const float* __restrict__ su = src.u + static_cast<size_t>(blockIdx.z) * src.stride;
    const float* __restrict__ sv = src.v + static_cast<size_t>(blockIdx.z) * src.stride;
    float* __restrict__ du = dst.u + static_cast<size_t>(blockIdx.z) * dst.stride;
    float* __restrict__ dv = dst.v + static_cast<size_t>(blockIdx.z) * dst.stride;
    const int gx = pixel_column();
    unsigned holes = 0;
    if (gx < w) {
#pragma unroll
        for (int r = 0; r < kPropagateRows; ++r) {
            const int gy = static_cast<int>(pixel_row(kPropagateRows, r));
            if (gy >= h) break;
            const unsigned long long key = keys[static_cast<size_t>(gy) * static_cast<size_t>(w) + static_cast<size_t>(gx)];
            float ou = __uint_as_float(0x7fc00000u), ov = __uint_as_float(0x7fc00000u);
            if (key != 0ull) {  // (a key is never zero: i <= 2^32 - 2, so its low word is at least 1)
                const unsigned i = 0xFFFFFFFFu - static_cast<unsigned>(key & 0xFFFFFFFFull);
                const int sy = static_cast<int>(i / static_cast<unsigned>(w)), sx = static_cast<int>(i % static_cast<unsigned>(w));
                const Offset s = pixel_offset<Offset>(sx, sy, src.pitch);
                ou = load_at(su, s);
                ov = load_at(sv, s);
            } else {
                ++holes;
            }
            const Offset d = pixel_offset<Offset>(gx, gy, dst.pitch);
            store_at(du, d, ou);
            store_at(dv, d, ov);
        }
    }
    if (record_base == nullptr) return;
    unsigned long long* record = record_base + static_cast<size_t>(blockIdx.z) * kRecordSlots;
    wave_add(record + kHoles, holes);
    if (count_unfilled) wave_add(record + kUnfilled, holes);  // no fill pass follows
}

// One fill pass: a pixel that is not finite in both components and has a neighbour that is takes the neighbours' mean.
template <typename Offset>
__global__ __launch_bounds__(flow2d::kPixelBlockX* flow2d::kPixelBlockY) void propagate_fill_kernel(ConstPlanePair src, PlanePair dst,
                                                                                                     unsigned long long* record_base,
                                                                                                     int w, int h, int last)
{
    const float* __restrict__ su = src.u + static_cast<size_t>(blockIdx.z) * src.stride;
    const float* __restrict__ sv = src.v + static_cast<size_t>(blockIdx.z) * src.stride;
    float* __restrict__ du = dst.u + static_cast<size_t>(blockIdx.z) * dst.stride;
    float* __restrict__ dv = dst.v + static_cast<size_t>(blockIdx.z) * dst.stride;
    const int gx = pixel_column();
    unsigned filled = 0, unfilled = 0;
    if (gx < w) {
#pragma unroll
        for (int r = 0; r < kPropagateRows; ++r) {
            const int gy = static_cast<int>(pixel_row(kPropagateRows, r));
            if (gy >= h) break;
            const Offset s = pixel_offset<Offset>(gx, gy, src.pitch);
            float ou = load_at(su, s), ov = load_at(sv, s);
            if (!both_finite(ou, ov)) {
                float sum_u = 0.f, sum_v = 0.f, n = 0.f;
                // (-1,-1), (0,-1), (1,-1), (-1,0), (1,0), (-1,1), (0,1), (1,1)
#pragma unroll
                for (int j = -1; j <= 1; ++j) {
#pragma unroll
                    for (int i = -1; i <= 1; ++i) {
                        if (i == 0 && j == 0) continue;
                        const int nx = gx + i, ny = gy + j;
                        if (nx < 0 || nx >= w || ny < 0 || ny >= h) continue;
                        const Offset o = pixel_offset<Offset>(nx, ny, src.pitch);
                        const float nu = load_at(su, o), nv = load_at(sv, o);
                        if (both_finite(nu, nv)) {
                            sum_u += nu;
                            sum_v += nv;
                            n += 1.f;
                        }
                    }
                }
                if (n > 0.f) {
                    ou = sum_u / n;
                    ov = sum_v / n;
                    ++filled;
                } else {
                    ++unfilled;
                }
            }
            const Offset d = pixel_offset<Offset>(gx, gy, dst.pitch);
            store_at(du, d, ou);
            store_at(dv, d, ov);
        }
    }
    if (record_base == nullptr) return;
    unsigned long long* record = record_base + static_cast<size_t>(blockIdx.z) * kRecordSlots;
    wave_add(record + kFilled, filled);
    if (last) wave_add(record + kUnfilled, unfilled);
}

inline size_t round_up_16(size_t bytes) { return (bytes + 15) & ~static_cast<size_t>(15); }
// the workspace: the keys of every instance (one memset), then two dense planes per instance
inline size_t keys_bytes(size_t width, size_t height, size_t instances) { return round_up_16(width * height * instances * sizeof(unsigned long long)); }

}  // namespace

extern "C" {

size_t flow2d_propagate_flow_workspace_bytes(size_t width, size_t height, size_t instances)
{
    if (width == 0 || height == 0 || instances == 0) return 0;
    return keys_bytes(width, height, instances) + round_up_16(width * height * instances * 2 * sizeof(float));
}

int flow2d_propagate_flow_2d(flow2d_context* ctx, const float* flow_u, const float* flow_v, const float* mask, const float* frame_from,
                             const float* frame_to, size_t width, size_t height, size_t pitch_bytes, float step, float photo_scale,
                             int fill_passes, float* out_u, float* out_v, unsigned long long* record, void* workspace)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    const void* required[] = {flow_u, flow_v, out_u, out_v};
    for (const void* p : required)
        if (!flow2d::plane_args_ok(p, width, height, pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    const void* optional[] = {mask, frame_from, frame_to};
    for (const void* p : optional)
        if (p && !flow2d::plane_args_ok(p, width, height, pitch_bytes)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if ((frame_from == nullptr) != (frame_to == nullptr)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (width * height > 0xFFFFFFFFull) return FLOW2D_ERR_INVALID_ARGUMENT;  // the key holds a 32-bit source index
    if (!std::isfinite(step) || step == 0.f || !std::isfinite(photo_scale) || photo_scale < 0.f) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (fill_passes < 0 || fill_passes > FLOW2D_PROPAGATE_MAX_FILL) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (record && (reinterpret_cast<uintptr_t>(record) % alignof(unsigned long long)) != 0) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) % 16) != 0) return FLOW2D_ERR_INVALID_ARGUMENT;
    // the kernels mark every plane __restrict__: no written byte range may meet a read one or another written one
    const size_t plane_bytes = height * pitch_bytes;
    auto aliased = [&](size_t span, size_t instances) {
        const flow2d::ByteRange written[] = {{out_u, span}, {out_v, span}, {record, instances * FLOW2D_PROPAGATE_RECORD_BYTES},
                                             {workspace, flow2d_propagate_flow_workspace_bytes(width, height, instances)}};
        const flow2d::ByteRange read[] = {{flow_u, span}, {flow_v, span}, {mask, span}, {frame_from, span}, {frame_to, span}};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(plane_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t instances = ctx->batch_count;
    if (aliased(flow2d::batch_span(ctx, plane_bytes), instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    const size_t keys_size = keys_bytes(width, height, instances);
    unsigned long long* keys = static_cast<unsigned long long*>(workspace);
    float* dense = reinterpret_cast<float*>(static_cast<char*>(workspace) + keys_size);
    const size_t dense_plane = width * height;  // floats
    FLOW2D_HIP_TRY(hipMemsetAsync(keys, 0, width * height * instances * sizeof(unsigned long long), ctx->stream));
    if (record) FLOW2D_HIP_TRY(hipMemsetAsync(record, 0, instances * FLOW2D_PROPAGATE_RECORD_BYTES, ctx->stream));
    const bool frames = frame_from != nullptr && photo_scale != 0.f;
    const int w = static_cast<int>(width), h = static_cast<int>(height), pitch = static_cast<int>(pitch_bytes / 4);
    const SplatArgs a = {flow_u, flow_v, mask, frames ? frame_from : nullptr, frames ? frame_to : nullptr, keys, record, w, h, pitch, step,
                         photo_scale};
    const BatchArg batch = flow2d::batch_arg(ctx, 1);
    const dim3 grid = flow2d::pixel_grid(ctx, width, height, kPropagateRows), block = flow2d::pixel_block();
    const ConstPlanePair flow = {flow_u, flow_v, pitch, batch.stride};
    const PlanePair out = {out_u, out_v, pitch, batch.stride};
    const PlanePair spare = {dense, dense + dense_plane, w, static_cast<unsigned long long>(2 * dense_plane)};
    auto as_const = [](const PlanePair& p) { return ConstPlanePair{p.u, p.v, p.pitch, p.stride}; };
    // (the largest offset a lane forms is below height * pitch floats: the dense planes are no larger than the pitched ones)
    flow2d::launch_by_span(plane_bytes, [&](auto offset) {
        using Offset = decltype(offset);
        if (mask && frames)
            propagate_splat_kernel<Offset, true, true><<<grid, block, 0, ctx->stream>>>(a, batch);
        else if (mask)
            propagate_splat_kernel<Offset, true, false><<<grid, block, 0, ctx->stream>>>(a, batch);
        else if (frames)
            propagate_splat_kernel<Offset, false, true><<<grid, block, 0, ctx->stream>>>(a, batch);
        else
            propagate_splat_kernel<Offset, false, false><<<grid, block, 0, ctx->stream>>>(a, batch);
        // pass k of n writes the output when n - k is even: the last pass (k = n) always does
        PlanePair to = (fill_passes % 2 == 0) ? out : spare;
        propagate_resolve_kernel<Offset><<<grid, block, 0, ctx->stream>>>(keys, flow, to, record, w, h, fill_passes == 0 ? 1 : 0);
        for (int k = 1; k <= fill_passes; ++k) {
            const PlanePair from = to;
            to = ((fill_passes - k) % 2 == 0) ? out : spare;
            propagate_fill_kernel<Offset><<<grid, block, 0, ctx->stream>>>(as_const(from), to, record, w, h, k == fill_passes ? 1 : 0);
        }
    });
    FLOW2D_CHECK_LAUNCH();
    return FLOW2D_OK;
}

}  // extern "C"

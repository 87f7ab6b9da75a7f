// Deformation analysis of a flow for gfx950: divergence, vorticity, dilatation, the strain tensor and its principal values
// from masked differences, with ordered statistics.  No reference counterpart.
//
// The normative definition is the one of flow2d_deformation_2d in flow2d_c_abi.h.  Built -ffp-contract=off: every plane
// follows that definition bit for bit.
//
// A masked stencil over two planes with up to nine fused outputs and a reduction.  Geometry of plane_sample.hpp (64 x 4
// threads, one column per lane, 32-bit byte offsets against scalar bases where the plane's span allows), but a thread takes
// kDeformRows CONSECUTIVE rows: it reads u, v and the mask of its column once for those rows and for one halo row above and
// below, and the y differences come out of registers.  The x neighbours are loads of the columns to the left and right: the
// same 128-byte lines the wave's centre load has just brought into the CU's L1, so they cost load instructions, not HBM
// traffic, and need neither a cross-lane step nor a special case at the ends of a wave.  Every load of a thread is issued
// before its first store.  Memory-bound: per pixel 8 bytes read (12 with a mask) and 4 written per requested plane.
//
// What is not requested costs nothing: the kernel is instantiated for three sets of quantities (first-order only; with the
// strain tensor; with its principal values, which need the square root), the largest once more with statistics, and a store
// to a plane the caller left out is skipped by a uniform branch.  Statistics are the two-launch ordered reduction of
// flow_error.hip (ordered_reduce.hpp): one slab per workgroup, then one workgroup per instance adds the slabs in block order.
#include <cfloat>
#include <cmath>

#include "node_grid.hpp"
#include "plane_sample.hpp"
#include "strain_sums.hpp"

namespace {

constexpr int kDeformRows = 4;  // consecutive rows per thread
constexpr int kBlockCols = flow2d::kPixelBlockX;                 // 64
constexpr int kBlockRows = flow2d::kPixelBlockY * kDeformRows;   // 16

enum Set { kFirstOrder = 0, kStrain = 1, kPrincipal = 2 };

struct DeformArgs {
    const float *u, *v, *mask;
    int w, h, pitch, measure;
};

// ok(q) of the definition; m < 0.5f after the clamp is m < 0.5f before it (a NaN fails, a negative value passes)
template <bool HasMask>
__device__ __forceinline__ bool vector_ok(float u, float v, float m)
{
    return fabsf(u) <= 1e9f && fabsf(v) <= 1e9f && (!HasMask || m < 0.5f);
}

// The masked difference along one axis: lo / hi are the neighbours' values, has_lo / has_hi whether they are ok.  The
// unused operand of a one-sided form may hold anything (a NaN, a masked vector): it is selected away, never combined.
__device__ __forceinline__ float masked_difference(float lo, float mid, float hi, bool has_lo, bool has_hi)
{
    const float both = (hi - lo) * 0.5f, forward = hi - mid, backward = mid - lo;
    return has_lo ? (has_hi ? both : backward) : forward;
}

template <typename Offset, bool HasMask, int kSet, bool Stats>
__global__ __launch_bounds__(256) void deformation_kernel(DeformArgs in, float* __restrict__ o_div, float* __restrict__ o_vort,
                                                          float* __restrict__ o_dil, float* __restrict__ o_exx,
                                                          float* __restrict__ o_eyy, float* __restrict__ o_exy,
                                                          float* __restrict__ o_e1, float* __restrict__ o_e2,
                                                          float* __restrict__ o_shear, StrainSums* __restrict__ partials,
                                                          BatchArg batch)
{
    static_assert(!Stats || kSet == kPrincipal, "the record holds the principal strains");
    const size_t inst = batch_offset(batch);
    const float* __restrict__ pu = in.u + inst;
    const float* __restrict__ pv = in.v + inst;
    const float* __restrict__ pm = HasMask ? in.mask + inst : nullptr;
    const int w = in.w, h = in.h, pitch = in.pitch;
    const int gx = pixel_column();
    const int y0 = (blockIdx.y * flow2d::kPixelBlockY + threadIdx.y) * kDeformRows;

    StrainSums acc;
    acc.clear();

    if (gx < w && y0 < h) {
        // every index is clamped into the frame before it is loaded: what lies outside is not ok and is selected away
        const int xl = max(gx - 1, 0), xr = min(gx + 1, w - 1);
        float cu[kDeformRows + 2], cv[kDeformRows + 2];
        bool cok[kDeformRows + 2];
#pragma unroll
        for (int j = 0; j < kDeformRows + 2; ++j) {
            const int y = y0 - 1 + j, yc = min(max(y, 0), h - 1);
            const Offset c = pixel_offset<Offset>(gx, yc, pitch);
            cu[j] = load_at(pu, c);
            cv[j] = load_at(pv, c);
            const float m = HasMask ? load_at(pm, c) : 0.f;
            cok[j] = y >= 0 && y < h && vector_ok<HasMask>(cu[j], cv[j], m);
        }
        float lu[kDeformRows], lv[kDeformRows], ru[kDeformRows], rv[kDeformRows];
        bool lok[kDeformRows], rok[kDeformRows];
#pragma unroll
        for (int i = 0; i < kDeformRows; ++i) {
            const int yc = min(y0 + i, h - 1);
            const Offset l = pixel_offset<Offset>(xl, yc, pitch), r = pixel_offset<Offset>(xr, yc, pitch);
            lu[i] = load_at(pu, l);
            lv[i] = load_at(pv, l);
            ru[i] = load_at(pu, r);
            rv[i] = load_at(pv, r);
            const float ml = HasMask ? load_at(pm, l) : 0.f, mr = HasMask ? load_at(pm, r) : 0.f;
            lok[i] = gx > 0 && vector_ok<HasMask>(lu[i], lv[i], ml);
            rok[i] = gx + 1 < w && vector_ok<HasMask>(ru[i], rv[i], mr);
        }
        float* const planes[9] = {o_div, o_vort, o_dil, o_exx, o_eyy, o_exy, o_e1, o_e2, o_shear};
#pragma unroll
        for (int i = 0; i < kDeformRows; ++i) {
            const int y = y0 + i;
            if (y >= h) break;
            const bool up = cok[i], down = cok[i + 2];
            const bool valid = cok[i + 1] && (lok[i] || rok[i]) && (up || down);
            const float a = masked_difference(lu[i], cu[i + 1], ru[i], lok[i], rok[i]);
            const float c = masked_difference(lv[i], cv[i + 1], rv[i], lok[i], rok[i]);
            const float b = masked_difference(cu[i], cu[i + 1], cu[i + 2], up, down);
            const float d = masked_difference(cv[i], cv[i + 1], cv[i + 2], up, down);
            float q[9];
            q[0] = a + d;
            q[1] = c - b;
            q[2] = (a + d) + (a * d - b * c);
            if (kSet >= kStrain) {
                float exx = a, eyy = d, exy = 0.5f * (b + c);
                if (in.measure == FLOW2D_STRAIN_GREEN_LAGRANGE) {
                    exx = a + 0.5f * (a * a + c * c);
                    eyy = d + 0.5f * (b * b + d * d);
                    exy = 0.5f * ((b + c) + (a * b + c * d));
                }
                q[3] = exx;
                q[4] = eyy;
                q[5] = exy;
                if (kSet >= kPrincipal) {
                    const float mean = 0.5f * (exx + eyy), half = 0.5f * (exx - eyy);
                    const float shear = sqrtf(half * half + exy * exy);
                    q[6] = mean + shear;
                    q[7] = mean - shear;
                    q[8] = shear;
                }
            }
            const Offset o = pixel_offset<Offset>(gx, y, pitch);
            constexpr int kPlanes = kSet == kFirstOrder ? 3 : kSet == kStrain ? 6 : 9;
#pragma unroll
            for (int k = 0; k < kPlanes; ++k)
                if (planes[k]) store_at(planes[k] + inst, o, valid ? q[k] : quiet_nan());
            if (Stats) {
                // predicated, not branched; adding +0.0 leaves a sum's bits as they are (the sums start at +0 and never become -0)
                const float x[kStrainQuantities] = {q[0], q[1], q[2], q[6], q[7], q[8]};
#pragma unroll
                for (int k = 0; k < kStrainQuantities; ++k) {
                    const double t = valid ? static_cast<double>(x[k]) : 0.0;
                    acc.sum[k] += t;
                    acc.sum_sq[k] += t * t;
                    acc.min[k] = (valid && x[k] < acc.min[k]) ? x[k] : acc.min[k];
                    acc.max[k] = (valid && x[k] > acc.max[k]) ? x[k] : acc.max[k];
                }
                acc.valid += valid;
                acc.invalid += !valid;
            }
        }
    }
    if (Stats) {
        // (every thread of the workgroup arrives here: the reduction holds a barrier)
        if (workgroup_reduce<flow2d::kPixelBlockY>(acc, threadIdx.x, threadIdx.y))
            partials[static_cast<size_t>(blockIdx.z) * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] = acc;
    }
}

inline size_t partial_blocks(size_t width, size_t height)
{
    return static_cast<size_t>(flow2d::div_up(width, kBlockCols)) * flow2d::div_up(height, kBlockRows);
}

template <typename Offset, bool HasMask, int kSet, bool Stats>
void launch_set(flow2d_context* ctx, const DeformArgs& in, const flow2d_deformation_planes& p, StrainSums* partials, size_t width,
                size_t height)
{
    deformation_kernel<Offset, HasMask, kSet, Stats>
        <<<flow2d::pixel_grid(ctx, width, height, kDeformRows), flow2d::pixel_block(), 0, ctx->stream>>>(
            in, p.divergence, p.vorticity, p.dilatation, p.exx, p.eyy, p.exy, p.e1, p.e2, p.max_shear, partials,
            flow2d::batch_arg(ctx, 1));
}

template <typename Offset, bool HasMask>
void launch_mask(flow2d_context* ctx, const DeformArgs& in, const flow2d_deformation_planes& p, StrainSums* partials, size_t width,
                 size_t height)
{
    if (partials)
        launch_set<Offset, HasMask, kPrincipal, true>(ctx, in, p, partials, width, height);
    else if (p.e1 || p.e2 || p.max_shear)
        launch_set<Offset, HasMask, kPrincipal, false>(ctx, in, p, nullptr, width, height);
    else if (p.exx || p.eyy || p.exy)
        launch_set<Offset, HasMask, kStrain, false>(ctx, in, p, nullptr, width, height);
    else
        launch_set<Offset, HasMask, kFirstOrder, false>(ctx, in, p, nullptr, width, height);
}

}  // namespace

extern "C" {

size_t flow2d_deformation_workspace_bytes(size_t width, size_t height, size_t instances)
{
    if (width == 0 || height == 0 || instances == 0) return 0;
    return partial_blocks(width, height) * instances * sizeof(StrainSums);
}

int flow2d_deformation_2d(flow2d_context* ctx, const float* flow_u, const float* flow_v, const float* mask, size_t width,
                          size_t height, size_t pitch_bytes, int measure, const flow2d_deformation_planes* out,
                          flow2d_deformation_stats* stats, void* workspace, size_t workspace_bytes)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    const flow2d_deformation_planes p = out ? *out : flow2d_deformation_planes{};
    float* const planes[9] = {p.divergence, p.vorticity, p.dilatation, p.exx, p.eyy, p.exy, p.e1, p.e2, p.max_shear};
    if (!flow2d::planes_ok({flow_u, flow_v},
                           {mask, planes[0], planes[1], planes[2], planes[3], planes[4], planes[5], planes[6], planes[7], planes[8]},
                           width, height, pitch_bytes))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (width < 2 || height < 2) return FLOW2D_ERR_INVALID_ARGUMENT;  // no derivative exists
    if (measure != FLOW2D_STRAIN_SMALL && measure != FLOW2D_STRAIN_GREEN_LAGRANGE) return FLOW2D_ERR_INVALID_ARGUMENT;
    bool any = stats != nullptr;
    for (float* q : planes) any = any || q != nullptr;
    if (!any) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::record_aligned(stats) || (reinterpret_cast<uintptr_t>(workspace) % 16) != 0) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (stats && (!workspace || workspace_bytes < flow2d_deformation_workspace_bytes(width, height, 1)))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    // the kernel marks every plane __restrict__: no written byte range may meet a read one or another written one.  Without
    // statistics the workspace is not touched and takes no part.
    auto aliased = [&](size_t span, size_t instances) {
        flow2d::ByteRange written[11];
        for (int k = 0; k < 9; ++k) written[k] = {planes[k], span};
        written[9] = {stats, instances * sizeof(flow2d_deformation_stats)};
        written[10] = {stats ? workspace : nullptr, workspace_bytes};
        const flow2d::ByteRange read[] = {{flow_u, span}, {flow_v, span}, {mask, span}};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(height * pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t instances = ctx->batch_count;
    if (stats && workspace_bytes < flow2d_deformation_workspace_bytes(width, height, instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (aliased(flow2d::batch_span(ctx, height * pitch_bytes), instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    const DeformArgs in = {flow_u, flow_v, mask, static_cast<int>(width), static_cast<int>(height),
                           static_cast<int>(pitch_bytes / 4), measure};
    StrainSums* partials = stats ? static_cast<StrainSums*>(workspace) : nullptr;
    // (the largest offset a lane forms is below height * pitch_bytes)
    flow2d::launch_by_span(height * pitch_bytes, [&](auto offset) {
        using Offset = decltype(offset);
        if (mask)
            launch_mask<Offset, true>(ctx, in, p, partials, width, height);
        else
            launch_mask<Offset, false>(ctx, in, p, partials, width, height);
    });
    FLOW2D_CHECK_LAUNCH();
    if (stats) {
        strain_final_kernel<<<dim3(static_cast<unsigned>(instances)), dim3(kStrainFinalThreads), 0, ctx->stream>>>(
            partials, static_cast<unsigned>(partial_blocks(width, height)), stats);
        FLOW2D_CHECK_LAUNCH();
    }
    return FLOW2D_OK;
}

}  // extern "C"

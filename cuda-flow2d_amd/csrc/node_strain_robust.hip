// Robust strain windows on the node grid of a DIC field for gfx950: the window fit of flow2d_node_strain_2d as iteratively
// reweighted least squares with a Cauchy weight (Holland & Welsch, Commun. Stat. 1977), so that a node which converged to a wrong
// place does not bend the windows that hold it, with three diagnostic planes that say which nodes were left out.  No reference
// counterpart.
//
// The normative definition is the one of flow2d_node_strain_robust_2d in flow2d_c_abi.h, in IEEE double.  Built
// -ffp-contract=off.
//
// The geometry is node_strain.hip's: one thread per node on the 64 x 4 block, the (64 + 2m) x (4 + 2m) tile of u, v and the
// usable flag staged in LDS once.  Every pass walks the window again from the tile: K + 1 fits and one walk for the residuals
// of the last, K + 2 walks in all.  A tap's weight is recomputed from the previous pass's coefficients as it is met -- no weight
// is stored, there is no per-tap array.  The weighted monomial sums S[p][q] = sum of w * di^p dj^q, p + q <= 2 * order, are
// doubles (6 or 15); with w = 1 they are sums of integers below 2^53 and therefore the sibling's.  Factorisation and solves are
// small_cholesky.hpp's, per thread, every loop over k unrolled: the arrays live in registers (no scratch;
// profiles/robust_strain/README.md has the register counts).
//
// Statistics are the two-launch ordered reduction of ordered_reduce.hpp with slabs of RobustStrainSums.
#include <cfloat>
#include <cmath>

#include "node_strain_common.hpp"
#include "small_cholesky.hpp"

namespace {

// nodes with a rejected tap, rejected taps, suspect nodes, over the nodes whose passes ran to the end: reserved[3 .. 5] of the record
constexpr int kRobustCounts = 3;

// NodeStrainSums with the three counts of the robust fit.
struct RobustStrainSums : NodeStrainSums {
    unsigned long long robust[kRobustCounts];
    unsigned long long pad2;

    __device__ __forceinline__ void clear()
    {
        NodeStrainSums::clear();
        pad2 = 0;
#pragma unroll
        for (int k = 0; k < kRobustCounts; ++k) robust[k] = 0;
    }
    __device__ __forceinline__ void combine(const RobustStrainSums& q)
    {
        NodeStrainSums::combine(q);
#pragma unroll
        for (int k = 0; k < kRobustCounts; ++k) robust[k] += q.robust[k];
    }
    __device__ __forceinline__ void across_lanes()
    {
        NodeStrainSums::across_lanes();
#pragma unroll
        for (int k = 0; k < kRobustCounts; ++k) robust[k] = wave_sum(robust[k]);
    }
    __device__ __forceinline__ void fill(flow2d_deformation_stats& rec) const
    {
        NodeStrainSums::fill(rec);
        for (int k = 0; k < kRobustCounts; ++k) rec.reserved[kReasons + k] = robust[k];
    }
};
static_assert(sizeof(RobustStrainSums) == 224, "flow2d_node_strain_robust_workspace_bytes counts slabs of 224 bytes");

struct RobustArgs {
    const float *u, *v, *state;  // state: null = absent
    float* out[9];               // the planes of flow2d_deformation_planes, null = not requested
    float* diag[3];              // residual, rejected, centre, null = not requested
    int nw, nh, npitch;
    int s, window, min_nodes, measure, passes;  // passes = K
    float min_state;
    double s2;  // sigma * sigma
};

template <int Order, bool Stats>
__global__ __launch_bounds__(kThreads) void node_strain_robust_kernel(RobustArgs in, RobustStrainSums* __restrict__ partials, BatchArg batch)
{
    constexpr int K = Order == 2 ? 6 : 3;
    constexpr int kTile = kTileW * kTileH;
    __shared__ float tile_u[kTile], tile_v[kTile];
    __shared__ unsigned char tile_ok[kTile];

    const size_t inst = batch_offset(batch);
    const int i = pixel_column();
    const int j = static_cast<int>(pixel_row(1, 0));
    const bool active = i < in.nw && j < in.nh;
    const size_t at = node_at(inst, active ? i : 0, active ? j : 0, in.npitch);

    const int m = in.window;
    const int tw = flow2d::kPixelBlockX + 2 * m, th = flow2d::kPixelBlockY + 2 * m;
    const int x0 = static_cast<int>(blockIdx.x) * flow2d::kPixelBlockX - m;
    const int y0 = static_cast<int>(blockIdx.y) * flow2d::kPixelBlockY - m;
    const int tid = threadIdx.y * flow2d::kPixelBlockX + threadIdx.x;
    // (tw * th <= kTile: the entry refuses a window beyond kMaxWindow)
    for (int t = tid; t < tw * th; t += kThreads) {
        const int ty = t / tw, tx = t - ty * tw;
        const int x = x0 + tx, y = y0 + ty;
        float u = 0.f, v = 0.f;
        bool ok = false;
        if (x >= 0 && y >= 0 && x < in.nw && y < in.nh) {
            const size_t q = node_at(inst, x, y, in.npitch);
            u = in.u[q];
            v = in.v[q];
            ok = (in.state ? in.state[q] >= in.min_state : true) && finite(u) && finite(v);
        }
        tile_u[t] = u;
        tile_v[t] = v;
        tile_ok[t] = ok ? 1 : 0;
    }
    __syncthreads();

    int reason = kCentre;
    double ga = 0.0, gb = 0.0, gc = 0.0, gd = 0.0;
    int n = 0, kept = 0;
    bool finished = false;  // the passes ran to the end: the node is valid, or sparse by what it kept
    double kept_r2 = 0.0, centre_r2 = 0.0;
    const int centre = (static_cast<int>(threadIdx.y) + m) * tw + static_cast<int>(threadIdx.x) + m;
    if (active && tile_ok[centre]) {
        const double uc = static_cast<double>(tile_u[centre]), vc = static_cast<double>(tile_v[centre]);
        const double s2 = in.s2;
        double cu[K], cv[K];
#pragma unroll
        for (int a = 0; a < K; ++a) cu[a] = cv[a] = 0.0;
        reason = kValid;
        // walk t <= passes is the fit of pass t, weighted by the residuals of pass t - 1; the last walk only takes the residuals
        for (int t = 0; t <= in.passes + 1 && reason == kValid; ++t) {
            const bool fit = t <= in.passes;
            // the weighted monomial sums S[p][q] = sum of w * di^p dj^q, p + q <= 2 * Order, and the right-hand sides
            double S[5][5];
#pragma unroll
            for (int p = 0; p < 5; ++p)
#pragma unroll
                for (int q = 0; q < 5; ++q) S[p][q] = 0.0;
            double bu[K], bv[K];
#pragma unroll
            for (int a = 0; a < K; ++a) bu[a] = bv[a] = 0.0;
            int taps = 0;
            for (int dj = -m; dj <= m; ++dj) {
                const int row = centre + dj * tw;
                for (int di = -m; di <= m; ++di) {
                    if (!tile_ok[row + di]) continue;
                    const double wu = static_cast<double>(tile_u[row + di]) - uc;
                    const double wv = static_cast<double>(tile_v[row + di]) - vc;
                    int pi[5], pj[5];
                    pi[0] = pj[0] = 1;
#pragma unroll
                    for (int p = 1; p < 5; ++p) {
                        pi[p] = pi[p - 1] * di;
                        pj[p] = pj[p - 1] * dj;
                    }
                    double phi[K];
#pragma unroll
                    for (int a = 0; a < K; ++a) phi[a] = static_cast<double>(pi[exp_i(a)] * pj[exp_j(a)]);
                    double w = 1.0, r2 = 0.0;
                    if (t > 0) {
                        double fu = 0.0, fv = 0.0;
#pragma unroll
                        for (int a = 0; a < K; ++a) {
                            fu += cu[a] * phi[a];
                            fv += cv[a] * phi[a];
                        }
                        const double ru = wu - fu, rv = wv - fv;
                        r2 = ru * ru + rv * rv;
                        w = s2 / (s2 + r2);
                    }
                    if (fit) {
                        ++taps;
#pragma unroll
                        for (int p = 0; p <= 2 * Order; ++p)
#pragma unroll
                            for (int q = 0; p + q <= 2 * Order; ++q) S[p][q] += w * static_cast<double>(pi[p] * pj[q]);
#pragma unroll
                        for (int a = 0; a < K; ++a) {
                            const double wphi = w * phi[a];
                            bu[a] += wphi * wu;
                            bv[a] += wphi * wv;
                        }
                    } else {
                        if (r2 <= s2) {
                            ++kept;
                            kept_r2 += r2;
                        }
                        if (di == 0 && dj == 0) centre_r2 = r2;
                    }
                }
            }
            if (!fit) break;
            if (t == 0) {
                n = taps;
                if (!(n >= in.min_nodes)) {
                    reason = kSparse;
                    break;
                }
            }
            double L[K][K];
#pragma unroll
            for (int a = 0; a < K; ++a)
#pragma unroll
                for (int b = 0; b < K; ++b) L[a][b] = S[exp_i(a) + exp_i(b)][exp_j(a) + exp_j(b)];
            if (!factor<K>(L)) {
                reason = kDegenerate;
                break;
            }
            solve<K>(L, bu, cu);
            solve<K>(L, bv, cv);
        }
        if (reason == kValid) {
            finished = true;
            if (!(kept >= in.min_nodes)) {
                reason = kSparse;
            } else {
                const double s = static_cast<double>(in.s);
                ga = cu[1] / s;
                gb = cu[2] / s;
                gc = cv[1] / s;
                gd = cv[2] / s;
            }
        }
    }

    RobustStrainSums acc;
    if (Stats) acc.clear();
    if (active) {
        const bool valid = reason == kValid;
        float q[9];
        quantities(ga, gb, gc, gd, in.measure, q);
#pragma unroll
        for (int k = 0; k < 9; ++k)
            if (in.out[k]) in.out[k][at] = valid ? q[k] : quiet_nan();
        const int rejected = n - kept;
        const bool suspect = !(centre_r2 <= in.s2);
        if (in.diag[0]) in.diag[0][at] = valid ? static_cast<float>(sqrt(kept_r2 / static_cast<double>(kept))) : quiet_nan();
        if (in.diag[1]) in.diag[1][at] = valid ? static_cast<float>(rejected) : quiet_nan();
        if (in.diag[2]) in.diag[2][at] = valid ? static_cast<float>(sqrt(centre_r2)) : quiet_nan();
        if (Stats) {
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
#pragma unroll
            for (int k = 0; k < kReasons; ++k) acc.reasons[k] += reason == k;
            // (over the finished nodes, not the valid ones alone: a window that locks onto its outlier and comes out sparse is
            // what these counts are for)
            acc.robust[0] += finished && rejected > 0;
            acc.robust[1] += finished ? static_cast<unsigned long long>(rejected) : 0ull;
            acc.robust[2] += finished && suspect;
        }
    }
    if (Stats) {
        // (every thread of the workgroup arrives here: the reduction holds a barrier)
        if (workgroup_reduce<flow2d::kPixelBlockY>(acc, threadIdx.x, threadIdx.y))
            partials[static_cast<size_t>(blockIdx.z) * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] = acc;
    }
}

template <int Order>
void launch_order(flow2d_context* ctx, const RobustArgs& a, RobustStrainSums* partials, size_t nw, size_t nh)
{
    const dim3 grid = flow2d::pixel_grid(ctx, nw, nh, 1), block = flow2d::pixel_block();
    if (partials)
        node_strain_robust_kernel<Order, true><<<grid, block, 0, ctx->stream>>>(a, partials, flow2d::batch_arg(ctx, 1));
    else
        node_strain_robust_kernel<Order, false><<<grid, block, 0, ctx->stream>>>(a, nullptr, flow2d::batch_arg(ctx, 1));
}

}  // namespace

extern "C" {

size_t flow2d_node_strain_robust_workspace_bytes(size_t nw, size_t nh, size_t instances)
{
    if (nw == 0 || nh == 0 || instances == 0) return 0;
    return partial_blocks(nw, nh) * instances * sizeof(RobustStrainSums);
}

int flow2d_node_strain_robust_2d(flow2d_context* ctx, const float* node_u, const float* node_v, const float* node_state, size_t nw,
                                 size_t nh, size_t node_pitch_bytes, int spacing, int window, int order, int min_nodes, int min_state,
                                 int measure, float sigma, int iterations, const flow2d_deformation_planes* out,
                                 const flow2d_node_strain_diagnostics* diagnostics, flow2d_deformation_stats* stats, void* workspace,
                                 size_t workspace_bytes)
{
    if (ctx == nullptr) return FLOW2D_ERR_INVALID_ARGUMENT;
    // (every check that needs no context field comes first: they hold without a device)
    const flow2d_deformation_planes p = out ? *out : flow2d_deformation_planes{};
    const flow2d_node_strain_diagnostics g = diagnostics ? *diagnostics : flow2d_node_strain_diagnostics{};
    constexpr int kOut = 12;
    float* const planes[kOut] = {p.divergence, p.vorticity, p.dilatation, p.exx,      p.eyy,      p.exy,
                                 p.e1,         p.e2,        p.max_shear,  g.residual, g.rejected, g.centre};
    if (!flow2d::planes_ok({node_u, node_v},
                           {node_state, planes[0], planes[1], planes[2], planes[3], planes[4], planes[5], planes[6], planes[7], planes[8],
                            planes[9], planes[10], planes[11]},
                           nw, nh, node_pitch_bytes))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (spacing < 1 || spacing > FLOW2D_CORRELATION_MAX_SPACING || window < 1 || window > FLOW2D_NODE_STRAIN_MAX_WINDOW ||
        min_state < 0 || min_state > 1 || (measure != FLOW2D_STRAIN_SMALL && measure != FLOW2D_STRAIN_GREEN_LAGRANGE))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    if (order != 1 && order != 2) return FLOW2D_ERR_INVALID_ARGUMENT;
    const int k = order == 2 ? 6 : 3, side = 2 * window + 1;
    if (min_nodes < k || min_nodes > side * side) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!(std::isfinite(sigma) && sigma > 0.f) || iterations < 0 || iterations > FLOW2D_NODE_STRAIN_MAX_ITERATIONS)
        return FLOW2D_ERR_INVALID_ARGUMENT;
    bool any = stats != nullptr;
    for (float* q : planes) any = any || q != nullptr;
    if (!any) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::record_aligned(stats) || (reinterpret_cast<uintptr_t>(workspace) % 16) != 0) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (!flow2d::node_count_ok(nw, nh)) return FLOW2D_ERR_UNSUPPORTED;
    if (stats && (!workspace || workspace_bytes < flow2d_node_strain_robust_workspace_bytes(nw, nh, 1)))
        return FLOW2D_ERR_INVALID_ARGUMENT;
    // the kernel reads its neighbours' inputs while their threads write: no written byte range may meet a read one or another
    // written one.  Without statistics the workspace is not touched and takes no part.
    auto aliased = [&](size_t span, size_t instances) {
        flow2d::ByteRange written[kOut + 2];
        for (int q = 0; q < kOut; ++q) written[q] = {planes[q], span};
        written[kOut] = {stats, instances * sizeof(flow2d_deformation_stats)};
        written[kOut + 1] = {stats ? workspace : nullptr, workspace_bytes};
        const flow2d::ByteRange read[] = {{node_u, span}, {node_v, span}, {node_state, span}};
        return flow2d::any_overlap(written, read);
    };
    if (aliased(nh * node_pitch_bytes, 1)) return FLOW2D_ERR_INVALID_ARGUMENT;
    FLOW2D_ENTER(ctx);
    const size_t instances = ctx->batch_count;
    if (stats && workspace_bytes < flow2d_node_strain_robust_workspace_bytes(nw, nh, instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    if (aliased(flow2d::batch_span(ctx, nh * node_pitch_bytes), instances)) return FLOW2D_ERR_INVALID_ARGUMENT;
    RobustArgs a;
    a.u = node_u;
    a.v = node_v;
    a.state = node_state;
    for (int q = 0; q < 9; ++q) a.out[q] = planes[q];
    for (int q = 0; q < 3; ++q) a.diag[q] = planes[9 + q];
    a.nw = static_cast<int>(nw);
    a.nh = static_cast<int>(nh);
    a.npitch = static_cast<int>(node_pitch_bytes / 4);
    a.s = spacing;
    a.window = window;
    a.min_nodes = min_nodes;
    a.measure = measure;
    a.passes = iterations;
    a.min_state = static_cast<float>(min_state);
    a.s2 = static_cast<double>(sigma) * static_cast<double>(sigma);
    RobustStrainSums* partials = stats ? static_cast<RobustStrainSums*>(workspace) : nullptr;
    if (order == 1)
        launch_order<1>(ctx, a, partials, nw, nh);
    else
        launch_order<2>(ctx, a, partials, nw, nh);
    FLOW2D_CHECK_LAUNCH();
    if (stats) {
        strain_final_kernel<<<dim3(static_cast<unsigned>(instances)), dim3(kStrainFinalThreads), 0, ctx->stream>>>(
            partials, static_cast<unsigned>(partial_blocks(nw, nh)), stats);
        FLOW2D_CHECK_LAUNCH();
    }
    return FLOW2D_OK;
}

}  // extern "C"
